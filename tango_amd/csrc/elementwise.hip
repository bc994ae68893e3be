// HBM-bound elementwise / layout / packing kernels of the Tango engine.
#include "common.h"

namespace tango {

// ------------------------------------------------------------------------------------------
// Fused classifier-free-guidance combine + scheduler step (models.py:244-249 +
// mustango/diffusers/src/diffusers/schedulers/scheduling_ddpm.py:254-349, scheduling_ddim.py:238-360).
// One thread per (sample, position): 8 channels.  FMA contraction is disabled to keep the reference's
// unfused mul/add order so the DDPM rule is bit-identical to the fp32 reference given equal inputs.
// coef[step] = {sqrt(abar_t), sqrt(1-abar_t), coef_x0, coef_xt, sigma, sqrt(abar_prev), dir_coef, 0}
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                           unsigned* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
    const unsigned n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    const unsigned n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float& n0, float& n1) {
  const float u1 = ((float)a + 1.0f) * 2.3283064365386963e-10f;  // (0,1]
  const float u2 = (float)b * 2.3283064365386963e-10f;
  const float r = sqrtf(-2.0f * __logf(u1));
  float s, c;
  __sincosf(6.283185307179586f * u2, &s, &c);
  n0 = r * c; n1 = r * s;
}

// four N(0,1) draws for channels 4*c4 .. 4*c4+3 of latent position hw of GLOBAL sample `sample` at loop index `step`:
// the Philox counter is (hw, c4, sample, step), the key is the 64-bit seed -> independent of batch split / GPU count
__device__ __forceinline__ void philox_normal4(int hw, int c4, int sample, int step, unsigned long long seed, float (&n)[4]) {
  unsigned r[4];
  philox4x32((unsigned)hw, (unsigned)c4, (unsigned)sample, (unsigned)step, (unsigned)seed, (unsigned)(seed >> 32), r);
  box_muller(r[0], r[1], n[0], n[1]);
  box_muller(r[2], r[3], n[2], n[3]);
}

// Masked-latent inpainting (audioldm/latent_diffusion/ddim.py:210-217): x = q * m + (1 - m) * x with q the fork's add_noise of the known
// latents, q = sqrt(abar_t) * x0 + sqrt(1 - abar_t) * n (scheduling_ddpm.py:351-371), both in the fork's unfused multiply / add order
__device__ __forceinline__ float inpaint_blend(float x, float x0, float n, float sa, float sb, float m) {
#pragma clang fp contract(off)
  const float t0 = sa * x0; const float t1 = sb * n; const float q = t0 + t1;
  const float u0 = q * m; const float om = 1.0f - m; const float u1 = om * x;
  return u0 + u1;
}
// the blend noise of loop index `step`: the step noise's Philox counter with bit 31 of the step word set (disjoint stream, same key)
__host__ __device__ __forceinline__ int blend_step_word(int step) { return (int)((unsigned)step | 0x80000000u); }

// blend of loop index `step` for channel c of (b, hw): injected noise or the Philox draw cached per 4 channels in nb
__device__ __forceinline__ float blend_at(const SchedParams& p, int step, int b, int hw, int c, int64_t o, float x, float m,
                                          float (&nb)[4]) {
  float n;
  if (p.blend_noise) {
    n = p.blend_noise[(int64_t)step * p.B * p.C * p.HW + o];
  } else {
    if ((c & 3) == 0) philox_normal4(hw, c >> 2, p.sample_offset + b, blend_step_word(step), p.seed, nb);
    n = nb[c & 3];
  }
  return inpaint_blend(x, p.x0[o], n, p.blend_coef[2 * step], p.blend_coef[2 * step + 1], m);
}

// ------------------------------------------------------------------------------------------
// Guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4; diffusers'
// guidance_rescale): per sample b, over the n = C * HW values of this step's model output,
//   cfg = u + g * (c - u)        s_b = std(c) / std(cfg)   (unbiased, n - 1)        v = phi * (cfg * s_b) + (1 - phi) * cfg
// and the scheduler rule runs on v.  std(cfg) == 0 gives s_b = 1 (the formula would give NaN): the one deviation.
// Two launches in front of the guided update kernels:
//   guidance_stats_kernel  grid (ceil(HW / 256), B), one position (C channels of both halves) per thread: sum and sum of squares of
//     c - c[first] and cfg - cfg[first] (about the sample's first element, like the norm kernels), cfg evaluated with the update
//     kernel's own fp32 operations, accumulated in fp64; registers -> 64 lanes by shuffles -> 4 waves through LDS -> one partial.
//   guidance_scale_kernel  one thread per sample adds the partials in chunk order in fp64 and writes s_b as fp32.
// No atomics and a partition that depends on HW alone: s_b has the same bits whatever B, the sample's row or sample_offset.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float cfg_combine(float u, float c, float g) {
#pragma clang fp contract(off)
  const float dlt = c - u; const float gd = g * dlt;
  return u + gd;
}

__global__ __launch_bounds__(kGuideChunk) void guidance_stats_kernel(const SchedParams* __restrict__ pp) {
  const SchedParams p = *pp;
  if (!(p.rescale > 0.f)) return;
  __shared__ double red[kGuideChunk / 64][4];
  const int b = blockIdx.y, hw = blockIdx.x * kGuideChunk + threadIdx.x;
  const int C = p.C;
  const float g = p.gtable[*p.step_ptr * p.B + b];
  const float* u0 = p.eps + (int64_t)b * p.HW * C;
  const float* c0 = p.eps + (int64_t)(p.B + b) * p.HW * C;
  const double pc = (double)c0[0], pg = (double)cfg_combine(u0[0], c0[0], g);
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (hw < p.HW) {
    const float* eu = u0 + (int64_t)hw * C;
    const float* ec = c0 + (int64_t)hw * C;
    for (int c = 0; c < C; ++c) {
      const double dc = (double)ec[c] - pc, dg = (double)cfg_combine(eu[c], ec[c], g) - pg;
      a[0] += dc; a[1] += dc * dc; a[2] += dg; a[3] += dg * dg;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    for (int o = 32; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o, 64);
  if ((threadIdx.x & 63) == 0)
    for (int k = 0; k < 4; ++k) red[threadIdx.x >> 6][k] = a[k];
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = red[0][threadIdx.x];
    for (int w = 1; w < kGuideChunk / 64; ++w) t += red[w][threadIdx.x];
    p.gpart[((int64_t)b * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(64) void guidance_scale_kernel(const SchedParams* __restrict__ pp, int chunks) {
  const SchedParams p = *pp;
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (!(p.rescale > 0.f) || b >= p.B) return;
  double t[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < chunks; ++j)
    for (int k = 0; k < 4; ++k) t[k] += p.gpart[((int64_t)b * chunks + j) * 4 + k];
  const double n = (double)p.C * (double)p.HW;
  const double vc = (t[1] - t[0] * t[0] / n) / (n - 1.0), vg = (t[3] - t[2] * t[2] / n) / (n - 1.0);
  p.gscale[b] = vg > 0.0 ? (float)(sqrt(vc > 0.0 ? vc : 0.0) / sqrt(vg)) : 1.0f;
}

int launch_guidance_stats(const SchedParams* dev_params, int B, int HW, hipStream_t s) {
  const int chunks = guidance_chunks(HW);
  hipLaunchKernelGGL(guidance_stats_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(kGuideChunk), 0, s, dev_params);
  TANGO_HIP(hipGetLastError());
  hipLaunchKernelGGL(guidance_scale_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, dev_params, chunks);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// the model output the guided kernels run the scheduler rule on: CFG (models.py:246) with the table's scale g, then the rescale above
// with s = gscale[b]; phi == 0 leaves cfg as it is.  1 - phi is an fp32 subtraction.
__device__ __forceinline__ float guided_output(float u, float c, float g, float s, float phi) {
#pragma clang fp contract(off)
  const float cfg = cfg_combine(u, c, g);
  if (!(phi > 0.f)) return cfg;
  const float r = cfg * s;
  const float t0 = phi * r; const float om = 1.0f - phi; const float t1 = om * cfg;
  return t0 + t1;
}

// The parameter block is read from DEVICE memory (wave-uniform scalar loads): the launch itself then carries only one
// pointer, so the captured hipGraph of a denoise step stays valid when the caller's latents / noise pointers, guidance
// or prediction type change between calls (engine.hip refreshes the block with one hipMemcpyAsync per call).
// MASK: the inpainting variant -- after the update, the blend of loop index step + 1 (none after the last step)
// GUIDED: the guidance scale comes from the block's table and the rescale is applied (the block has cfg = 1)
template <typename T, bool MASK = false, bool GUIDED = false>
__global__ __launch_bounds__(256) void sched_step_kernel(const SchedParams* __restrict__ pp) {
  // plain operators + contract(off): the HIP _rn intrinsics are inlined header operators that still fuse
#pragma clang fp contract(off)
  const SchedParams p = *pp;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.B * p.HW) return;
  const int b = idx / p.HW, hw = idx - b * p.HW;
  const int step = *p.step_ptr;
  const float* cf = p.coef + step * 8;
  const float sa = cf[0], sb = cf[1], c0 = cf[2], c1 = cf[3], sig = cf[4], sap = cf[5], dirc = cf[6];
  const int C = p.C;
  const float* eu = p.eps + ((int64_t)b * p.HW + hw) * C;
  const float* ec = p.cfg ? p.eps + ((int64_t)(p.B + b) * p.HW + hw) * C : nullptr;
  T* xo0 = (T*)p.xin + ((int64_t)b * p.HW + hw) * p.xin_ld;
  T* xo1 = p.cfg ? (T*)p.xin + ((int64_t)(p.B + b) * p.HW + hw) * p.xin_ld : nullptr;
  float nrm[4] = {0.f, 0.f, 0.f, 0.f};
  float nb[4] = {0.f, 0.f, 0.f, 0.f};
  const bool blend = MASK && step + 1 < p.num_steps;
  const float m = MASK ? p.mask[(int64_t)b * p.HW + hw] : 0.f;
  const float gg = GUIDED ? p.gtable[step * p.B + b] : 0.f;
  const float gs = GUIDED && p.rescale > 0.f ? p.gscale[b] : 1.f;
  for (int c = 0; c < C; ++c) {
    float* lp = p.lat + ((int64_t)b * C + c) * p.HW + hw;
    const float x = *lp;
    float v = eu[c];
    if constexpr (GUIDED) v = guided_output(v, ec[c], gg, gs, p.rescale);
    else if (p.cfg) { const float dlt = ec[c] - v; const float gd = p.guidance * dlt; v = v + gd; }   // models.py:246
    float x0;
    if (p.pred_type == 0) { const float m0 = sb * v; const float d0 = x - m0; x0 = d0 / sa; }   // epsilon
    else if (p.pred_type == 1) x0 = v;                                               // sample
    else { const float m0 = sa * x; const float m1 = sb * v; x0 = m0 - m1; }   // v_prediction
    if (p.clip) x0 = fminf(fmaxf(x0, -p.clip_range), p.clip_range);
    float prev;
    float nz = 0.f;
    if (sig > 0.f) {
      if (p.noise) {
        nz = p.noise[(int64_t)step * p.B * C * p.HW + ((int64_t)b * C + c) * p.HW + hw];
      } else {
        if ((c & 3) == 0) philox_normal4(hw, c >> 2, p.sample_offset + b, step, p.seed, nrm);   // one draw per 4 channels
        nz = nrm[c & 3];
      }
    }
    if (p.rule == 0) {
      { const float m0 = c0 * x0; const float m1 = c1 * x; prev = m0 + m1; }
      if (sig > 0.f) { const float m2 = sig * nz; prev = prev + m2; }
    } else {
      float e;
      if (p.pred_type == 0) e = v;
      else if (p.pred_type == 1) { const float m0 = sa * x0; const float d0 = x - m0; e = d0 / sb; }
      else { const float m0 = sa * v; const float m1 = sb * x; e = m0 + m1; }
      { const float m0 = sap * x0; const float m1 = dirc * e; prev = m0 + m1; }
      if (sig > 0.f) { const float m2 = sig * nz; prev = prev + m2; }
    }
    if constexpr (MASK) {
      if (blend) prev = blend_at(p, step + 1, b, hw, c, ((int64_t)b * C + c) * p.HW + hw, prev, m, nb);
    }
    *lp = prev;
    const T tv = from_f<T>(prev);
    xo0[c] = tv;
    if (xo1) xo1[c] = tv;
  }
  // the last workgroup to get here could bump the step counter, but every block of THIS launch and of the next UNet
  // launch reads it: the increment stays a separate 1-thread launch (captured in the same hipGraph, engine.hip)
}

// test hook: the N(0,1) draws sched_step_kernel makes at loop index `step` for samples [sample_offset, sample_offset + B)
__global__ __launch_bounds__(256) void philox_normal_kernel(float* __restrict__ out, int B, int C, int HW, int step,
                                                            unsigned long long seed, int sample_offset) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * HW) return;
  const int b = idx / HW, hw = idx - b * HW;
  float nrm[4];
  for (int c = 0; c < C; ++c) {
    if ((c & 3) == 0) philox_normal4(hw, c >> 2, sample_offset + b, step, seed, nrm);
    out[((int64_t)b * C + c) * HW + hw] = nrm[c & 3];
  }
}
int launch_philox_normal(float* out, int B, int C, int HW, int step, unsigned long long seed, int sample_offset, hipStream_t s,
                         bool blend) {
  hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)((B * HW + 255) / 256)), dim3(256), 0, s, out, B, C, HW,
                     blend ? blend_step_word(step) : step, seed, sample_offset);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// Fused latent encode of audio-to-audio editing (AudioLDM style_transfer, audioldm/pipeline.py:145-247): VAE moments
// [Bm][2C][HW] = [mean | logvar] -> the latents the truncated loop starts from, one launch.  Per element, each line in the
// reference's unfused multiply / add order (FMA contraction off):
//   lv = clamp(logvar, -30, 20); z = mean + exp(0.5 * lv) * eps    distributions.py:24-41 (posterior mode: z = mean)
//   z  = scale * z                                                 autoencoder.py:126-135 get_first_stage_encoding
//   if max over the sample |z| > clip_trigger: z = clamp(z, -clip_range, clip_range)          pipeline.py:209-210
//   xt = sa * z + sb * n                                           latent_diffusion/ddim.py:259-262 == the fork's add_noise
// The clip condition is PER SAMPLE.  The reference takes torch.max over the whole tensor, but its only caller repeats one clip
// `batchsize` times (pipeline.py:203-206), where the two definitions agree; per sample, the result does not depend on what else is in
// the batch or on how a batch is split.
// One workgroup per sample, two passes over its C * HW values: pass 1 computes z and reduces max |z| (wave shuffle, then LDS),
// pass 2 recomputes z -- the same instructions on the same inputs, hence the same bits -- clips and writes.  Recomputing costs
// a second read of the moments (256 KB per sample at the engine's size, L2-resident) and keeps the kernel free of a size limit.
// eps / n: injected [B][C][HW] or null -> philox_normal4 with bit 30 of the step word set (word 0 eps, word 1 n): disjoint from
// the step noise (bits 31, 30 clear) and from the blend noise (bit 31 set) while a loop has fewer than 2^30 steps.
// With sb == 0 and no injected n the second stream is not drawn at all (xt = sa * z + 0).
// Bm == 1: every sample reads clip 0's moments (one clip fans out to B samples with different draws).
// ------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int encode_step_word(int which) { return (int)(0x40000000u | (unsigned)which); }

struct LatentEncodeParams {
  const float* moments; float* z0; float* xt; const float* eps; const float* noise;
  int B, C, HW, moments_batch;
  float scale, clip_trigger, clip_range, sa, sb;
  int posterior_mode, sample_offset;
  unsigned long long seed;
};

// scale * posterior value of channel c at hw of the sample whose moments start at mom; e = the eps draw (unused in mode)
__device__ __forceinline__ float encode_z(const float* __restrict__ mom, int C, int HW, int c, int hw, float e, bool mode,
                                          float scale) {
#pragma clang fp contract(off)
  const float mean = mom[(int64_t)c * HW + hw];
  float z = mean;
  if (!mode) {
    const float lv = fminf(fmaxf(mom[(int64_t)(C + c) * HW + hw], -30.0f), 20.0f);
    const float h = 0.5f * lv;
    const float sd = expf(h);
    const float t = sd * e;
    z = mean + t;
  }
  return scale * z;
}

constexpr int kEncodeThreads = 1024;
__global__ __launch_bounds__(kEncodeThreads) void latent_encode_kernel(const LatentEncodeParams p) {
#pragma clang fp contract(off)
  __shared__ float red[kEncodeThreads / 64];
  const int b = blockIdx.x;
  const int C = p.C, HW = p.HW;
  const bool mode = p.posterior_mode != 0;
  const float* mom = p.moments + (p.moments_batch == 1 ? (int64_t)0 : (int64_t)b * 2 * C * HW);
  const int64_t base = (int64_t)b * C * HW;
  const int items = ((C + 3) >> 2) * HW;          // one item = 4 channels of one position (one Philox call per stream)
  const bool eps_philox = !mode && !p.eps;
  const bool n_philox = !p.noise && p.sb != 0.f;   // sb == 0 (the posterior alone, e.g. before an inversion): no draw, n = 0
  float amax = 0.f;
  for (int i = threadIdx.x; i < items; i += kEncodeThreads) {
    const int c4 = i / HW, hw = i - c4 * HW;
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    if (eps_philox) philox_normal4(hw, c4, p.sample_offset + b, encode_step_word(0), p.seed, e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 4 * c4 + k;
      if (c < C) {
        const float ev = (!mode && p.eps) ? p.eps[base + (int64_t)c * HW + hw] : e[k];
        amax = fmaxf(amax, fabsf(encode_z(mom, C, HW, c, hw, ev, mode, p.scale)));
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
  __syncthreads();
  float smax = red[0];
  for (int w = 1; w < kEncodeThreads / 64; ++w) smax = fmaxf(smax, red[w]);
  const bool clip = smax > p.clip_trigger;
  for (int i = threadIdx.x; i < items; i += kEncodeThreads) {
    const int c4 = i / HW, hw = i - c4 * HW;
    float e[4] = {0.f, 0.f, 0.f, 0.f}, n[4] = {0.f, 0.f, 0.f, 0.f};
    if (eps_philox) philox_normal4(hw, c4, p.sample_offset + b, encode_step_word(0), p.seed, e);
    if (n_philox) philox_normal4(hw, c4, p.sample_offset + b, encode_step_word(1), p.seed, n);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int c = 4 * c4 + k;
      if (c < C) {
        const int64_t o = base + (int64_t)c * HW + hw;
        const float ev = (!mode && p.eps) ? p.eps[o] : e[k];
        float z = encode_z(mom, C, HW, c, hw, ev, mode, p.scale);
        if (clip) z = fminf(fmaxf(z, -p.clip_range), p.clip_range);
        const float nv = p.noise ? p.noise[o] : n[k];
        const float t0 = p.sa * z; const float t1 = p.sb * nv;
        p.xt[o] = t0 + t1;
        if (p.z0) p.z0[o] = z;
      }
    }
  }
}

int launch_latent_encode(const float* moments, int moments_batch, float* z0, float* xt, const float* eps, const float* noise, int B,
                         int C, int HW, float scale, float clip_trigger, float clip_range, float sa, float sb, int posterior_mode,
                         unsigned long long seed, int sample_offset, hipStream_t s) {
  LatentEncodeParams p;
  p.moments = moments; p.z0 = z0; p.xt = xt; p.eps = eps; p.noise = noise;
  p.B = B; p.C = C; p.HW = HW; p.moments_batch = moments_batch;
  p.scale = scale; p.clip_trigger = clip_trigger; p.clip_range = clip_range; p.sa = sa; p.sb = sb;
  p.posterior_mode = posterior_mode; p.sample_offset = sample_offset; p.seed = seed;
  hipLaunchKernelGGL(latent_encode_kernel, dim3((unsigned)B), dim3(kEncodeThreads), 0, s, p);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// test hook: the draws of latent_encode_kernel's two Philox streams (which: 0 eps, 1 n), in philox_normal_kernel's layout
int launch_philox_normal_encode(float* out, int B, int C, int HW, int which, unsigned long long seed, int sample_offset,
                                hipStream_t s) {
  hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)((B * HW + 255) / 256)), dim3(256), 0, s, out, B, C, HW,
                     encode_step_word(which), seed, sample_offset);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// Fused CFG combine + multistep DPM-Solver / DPM-Solver++ update (rule 2; fork
// mustango/diffusers/src/diffusers/schedulers/scheduling_dpmsolver_multistep.py:220-495).  One thread per (sample, position),
// 8 channels.  Every scalar comes from the host table row (tango_amd/scheduler.py DPMSolverMultistepScheduler.coef_table,
// computed as the fork's own fp32 0-dim expressions), and the tensor expressions keep the fork's association order with FMA
// contraction off, so with fp32 inputs the step equals the fork's step() bit for bit.
// row = {alpha_s0, sigma_s0, kx, c0, c1, c2, 1/r0, 1/r1, r0/(r0+r1), 1/(r0+r1), order, algo, 0...}
// The converted output m0 of this step goes to ring slot step % 3; m1 / m2 (steps - 1, - 2) are read from the other two slots
// only when the row's order asks for them, i.e. only once an earlier step of the same loop has written them.  No noise term.
// ------------------------------------------------------------------------------------------
// MASK: the inpainting variant, as sched_step_kernel's (the blended sample is the next step's `sample`); GUIDED: as sched_step_kernel's
template <typename T, bool MASK = false, bool GUIDED = false>
__global__ __launch_bounds__(256) void sched_multistep_kernel(const SchedParams* __restrict__ pp) {
#pragma clang fp contract(off)
  const SchedParams p = *pp;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.B * p.HW) return;
  const int b = idx / p.HW, hw = idx - b * p.HW;
  const int step = *p.step_ptr;
  const float* cf = p.coef + (int64_t)step * p.coef_w;
  const float a_s0 = cf[0], s_s0 = cf[1], kx = cf[2], c0 = cf[3], c1 = cf[4], c2 = cf[5];
  const float ir0 = cf[6], ir1 = cf[7], q = cf[8], ir01 = cf[9];
  const int order = (int)cf[10];
  const int C = p.C;
  const int64_t slot = (int64_t)p.B * C * p.HW;
  float* r0 = p.ring + (int64_t)(step % 3) * slot;
  const float* r1 = p.ring + (int64_t)((step + 2) % 3) * slot;   // step - 1
  const float* r2 = p.ring + (int64_t)((step + 1) % 3) * slot;   // step - 2
  const float* eu = p.eps + ((int64_t)b * p.HW + hw) * C;
  const float* ec = p.cfg ? p.eps + ((int64_t)(p.B + b) * p.HW + hw) * C : nullptr;
  T* xo0 = (T*)p.xin + ((int64_t)b * p.HW + hw) * p.xin_ld;
  T* xo1 = p.cfg ? (T*)p.xin + ((int64_t)(p.B + b) * p.HW + hw) * p.xin_ld : nullptr;
  float nb[4] = {0.f, 0.f, 0.f, 0.f};
  const bool blend = MASK && step + 1 < p.num_steps;
  const float m = MASK ? p.mask[(int64_t)b * p.HW + hw] : 0.f;
  const float gg = GUIDED ? p.gtable[step * p.B + b] : 0.f;
  const float gs = GUIDED && p.rescale > 0.f ? p.gscale[b] : 1.f;
  for (int c = 0; c < C; ++c) {
    const int64_t o = ((int64_t)b * C + c) * p.HW + hw;
    const float x = p.lat[o];
    float v = eu[c];
    if constexpr (GUIDED) v = guided_output(v, ec[c], gg, gs, p.rescale);
    else if (p.cfg) { const float dlt = ec[c] - v; const float gd = p.guidance * dlt; v = v + gd; }   // models.py:246
    float m0;                                                                                  // convert_model_output
    if (p.algo == 0) {                                                                         // x0
      if (p.pred_type == 0) { const float t0 = s_s0 * v; const float d0 = x - t0; m0 = d0 / a_s0; }
      else if (p.pred_type == 1) m0 = v;
      else { const float t0 = a_s0 * x; const float t1 = s_s0 * v; m0 = t0 - t1; }
    } else {                                                                                   // eps
      if (p.pred_type == 0) m0 = v;
      else if (p.pred_type == 1) { const float t0 = a_s0 * v; const float d0 = x - t0; m0 = d0 / s_s0; }
      else { const float t0 = a_s0 * v; const float t1 = s_s0 * x; m0 = t0 + t1; }
    }
    float prev;
    { const float t0 = kx * x; const float t1 = c0 * m0; prev = t0 + t1; }
    if (order == 2) {
      const float m1 = r1[o];
      const float d = m0 - m1; const float D1 = ir0 * d;
      const float t2 = c1 * D1; prev = prev + t2;
    } else if (order == 3) {
      const float m1 = r1[o], m2 = r2[o];
      const float e0 = m0 - m1; const float D10 = ir0 * e0;
      const float e1 = m1 - m2; const float D11 = ir1 * e1;
      const float dd = D10 - D11;
      const float t3 = q * dd; const float D1 = D10 + t3;
      const float D2 = ir01 * dd;
      const float t4 = c1 * D1; prev = prev + t4;
      const float t5 = c2 * D2; prev = prev + t5;
    }
    r0[o] = m0;
    if constexpr (MASK) {
      if (blend) prev = blend_at(p, step + 1, b, hw, c, o, prev, m, nb);
    }
    p.lat[o] = prev;
    const T tv = from_f<T>(prev);
    xo0[c] = tv;
    if (xo1) xo1[c] = tv;
  }
}

// the blend of loop index 0, before the first UNet call (the engine launches it once per call, outside the captured step)
template <typename T>
__global__ __launch_bounds__(256) void inpaint_blend0_kernel(const SchedParams* __restrict__ pp) {
  const SchedParams p = *pp;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.B * p.HW) return;
  const int b = idx / p.HW, hw = idx - b * p.HW;
  const int C = p.C;
  T* xo0 = (T*)p.xin + ((int64_t)b * p.HW + hw) * p.xin_ld;
  T* xo1 = p.cfg ? (T*)p.xin + ((int64_t)(p.B + b) * p.HW + hw) * p.xin_ld : nullptr;
  const float m = p.mask[(int64_t)b * p.HW + hw];
  float nb[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    const int64_t o = ((int64_t)b * C + c) * p.HW + hw;
    const float x = blend_at(p, 0, b, hw, c, o, p.lat[o], m, nb);
    p.lat[o] = x;
    const T tv = from_f<T>(x);
    xo0[c] = tv;
    if (xo1) xo1[c] = tv;
  }
}

int launch_inpaint_blend0(int dtype, const SchedParams* dev_params, int max_positions, hipStream_t s) {
  const unsigned nb = (unsigned)((max_positions + 255) / 256);
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((inpaint_blend0_kernel<float>), dim3(nb), dim3(256), 0, s, dev_params); break;
    case DT_F16: hipLaunchKernelGGL((inpaint_blend0_kernel<f16>), dim3(nb), dim3(256), 0, s, dev_params); break;
    case DT_BF16: hipLaunchKernelGGL((inpaint_blend0_kernel<bf16>), dim3(nb), dim3(256), 0, s, dev_params); break;
    default: TANGO_FAIL("inpaint_blend0: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

template <bool MASK, bool GUIDED>
static int launch_sched_variant(int dtype, const SchedParams* dev_params, unsigned nb, hipStream_t s, int rule) {
  if (rule == 2) {
    switch (dtype) {
      case DT_F32: hipLaunchKernelGGL((sched_multistep_kernel<float, MASK, GUIDED>), dim3(nb), dim3(256), 0, s, dev_params); break;
      case DT_F16: hipLaunchKernelGGL((sched_multistep_kernel<f16, MASK, GUIDED>), dim3(nb), dim3(256), 0, s, dev_params); break;
      case DT_BF16: hipLaunchKernelGGL((sched_multistep_kernel<bf16, MASK, GUIDED>), dim3(nb), dim3(256), 0, s, dev_params); break;
      default: TANGO_FAIL("sched_multistep: bad dtype");
    }
  } else {
    switch (dtype) {
      case DT_F32: hipLaunchKernelGGL((sched_step_kernel<float, MASK, GUIDED>), dim3(nb), dim3(256), 0, s, dev_params); break;
      case DT_F16: hipLaunchKernelGGL((sched_step_kernel<f16, MASK, GUIDED>), dim3(nb), dim3(256), 0, s, dev_params); break;
      case DT_BF16: hipLaunchKernelGGL((sched_step_kernel<bf16, MASK, GUIDED>), dim3(nb), dim3(256), 0, s, dev_params); break;
      default: TANGO_FAIL("sched_step: bad dtype");
    }
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

int launch_sched_step(int dtype, const SchedParams* dev_params, int max_positions, hipStream_t s, int rule, bool masked, bool guided) {
  const unsigned nb = (unsigned)((max_positions + 255) / 256);   // >= B*HW of the block; surplus threads exit
  if (guided) return masked ? launch_sched_variant<true, true>(dtype, dev_params, nb, s, rule)
                            : launch_sched_variant<false, true>(dtype, dev_params, nb, s, rule);
  return masked ? launch_sched_variant<true, false>(dtype, dev_params, nb, s, rule)
                : launch_sched_variant<false, false>(dtype, dev_params, nb, s, rule);
}

__global__ void step_inc_kernel(int* sp) { if (threadIdx.x == 0 && blockIdx.x == 0) *sp = *sp + 1; }
int launch_step_inc(int* step_ptr, hipStream_t s) {
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(64), 0, s, step_ptr);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// layout conversions at the C-ABI boundary (reference tensors are NCHW fp32)
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t ld,
                                                           int B, int C, int HW, int rep, float scale) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * HW) return;
  const int b = (int)(idx / HW), hw = (int)(idx - (int64_t)b * HW);
  for (int c = 0; c < C; ++c) {
    const T v = from_f<T>(src[((int64_t)b * C + c) * HW + hw] * scale);
    for (int r = 0; r < rep; ++r) dst[(((int64_t)r * B + b) * HW + hw) * ld + c] = v;
  }
}
int launch_nchw_to_nhwc(int dtype, const float* src, void* dst, int64_t ld, int B, int C, int HW, int rep, float scale,
                        hipStream_t s) {
  const unsigned nb = (unsigned)(((int64_t)B * HW + 255) / 256);
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((nchw_to_nhwc_kernel<float>), dim3(nb), dim3(256), 0, s, src, (float*)dst, ld, B, C, HW, rep, scale); break;
    case DT_F16: hipLaunchKernelGGL((nchw_to_nhwc_kernel<f16>), dim3(nb), dim3(256), 0, s, src, (f16*)dst, ld, B, C, HW, rep, scale); break;
    case DT_BF16: hipLaunchKernelGGL((nchw_to_nhwc_kernel<bf16>), dim3(nb), dim3(256), 0, s, src, (bf16*)dst, ld, B, C, HW, rep, scale); break;
    default: TANGO_FAIL("nchw_to_nhwc: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const T* __restrict__ src, int64_t ld, float* __restrict__ dst, int B,
                                                           int C, int HW) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * HW) return;
  const int b = (int)(idx / HW), hw = (int)(idx - (int64_t)b * HW);
  for (int c = 0; c < C; ++c) dst[((int64_t)b * C + c) * HW + hw] = to_f(src[((int64_t)b * HW + hw) * ld + c]);
}
int launch_nhwc_to_nchw_f32(int dtype, const void* src, int64_t ld, float* dst, int B, int C, int HW, hipStream_t s) {
  const unsigned nb = (unsigned)(((int64_t)B * HW + 255) / 256);
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((nhwc_to_nchw_kernel<float>), dim3(nb), dim3(256), 0, s, (const float*)src, ld, dst, B, C, HW); break;
    case DT_F16: hipLaunchKernelGGL((nhwc_to_nchw_kernel<f16>), dim3(nb), dim3(256), 0, s, (const f16*)src, ld, dst, B, C, HW); break;
    case DT_BF16: hipLaunchKernelGGL((nhwc_to_nchw_kernel<bf16>), dim3(nb), dim3(256), 0, s, (const bf16*)src, ld, dst, B, C, HW); break;
    default: TANGO_FAIL("nhwc_to_nchw: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void cast_rows_kernel(const float* __restrict__ src, T* __restrict__ dst, int64_t ld,
                                                        int64_t rows, int C) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * C) return;
  const int64_t r = idx / C;
  const int c = (int)(idx - r * C);
  dst[r * ld + c] = from_f<T>(src[idx]);
}
int launch_cast_rows(int dtype, const float* src, void* dst, int64_t ld, int rows, int C, hipStream_t s) {
  const unsigned nb = (unsigned)(((int64_t)rows * C + 255) / 256);
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((cast_rows_kernel<float>), dim3(nb), dim3(256), 0, s, src, (float*)dst, ld, (int64_t)rows, C); break;
    case DT_F16: hipLaunchKernelGGL((cast_rows_kernel<f16>), dim3(nb), dim3(256), 0, s, src, (f16*)dst, ld, (int64_t)rows, C); break;
    case DT_BF16: hipLaunchKernelGGL((cast_rows_kernel<bf16>), dim3(nb), dim3(256), 0, s, src, (bf16*)dst, ld, (int64_t)rows, C); break;
    default: TANGO_FAIL("cast_rows: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

// im2col for the tiny-Cin 3x3 convs (UNet conv_in 8->320, VAE conv_in 8->512): K = 9*C padded to Kp.
template <typename T>
__global__ __launch_bounds__(256) void im2col3x3_kernel(const T* __restrict__ src, int64_t ld, T* __restrict__ dst, int64_t Kp,
                                                        int B, int H, int W, int C) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t total = (int64_t)B * H * W * Kp;
  if (idx >= total) return;
  const int64_t m = idx / Kp;
  const int k = (int)(idx - m * Kp);
  T v = from_f<T>(0.f);
  if (k < 9 * C) {
    const int tap = k / C, c = k - tap * C;
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    const int hw = H * W;
    const int b = (int)(m / hw);
    const int rem = (int)(m - (int64_t)b * hw);
    const int y = rem / W + dy, x = rem % W + dx;
    if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) v = src[(((int64_t)b * H + y) * W + x) * ld + c];
  }
  dst[idx] = v;
}
int launch_im2col3x3(int dtype, const void* src, int64_t ld, void* dst, int64_t Kp, int B, int H, int W, int C, hipStream_t s) {
  const unsigned nb = (unsigned)(((int64_t)B * H * W * Kp + 255) / 256);
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((im2col3x3_kernel<float>), dim3(nb), dim3(256), 0, s, (const float*)src, ld, (float*)dst, Kp, B, H, W, C); break;
    case DT_F16: hipLaunchKernelGGL((im2col3x3_kernel<f16>), dim3(nb), dim3(256), 0, s, (const f16*)src, ld, (f16*)dst, Kp, B, H, W, C); break;
    case DT_BF16: hipLaunchKernelGGL((im2col3x3_kernel<bf16>), dim3(nb), dim3(256), 0, s, (const bf16*)src, ld, (bf16*)dst, Kp, B, H, W, C); break;
    default: TANGO_FAIL("im2col: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

// y = act((a + b + c) * scale): HiFi-GAN "xs / num_kernels" + following leaky_relu (hifigan/models.py:153-161)
template <typename T>
__global__ __launch_bounds__(256) void avg3_act_kernel(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ c,
                                                       T* __restrict__ y, int64_t nvec, float scale, int act, float slope) {
  constexpr int EPV = 16 / (int)sizeof(T);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
    T ea[EPV], eb[EPV], ec[EPV], eo[EPV];
    __builtin_memcpy(ea, a + i * EPV, 16);
    __builtin_memcpy(eb, b + i * EPV, 16);
    __builtin_memcpy(ec, c + i * EPV, 16);
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      // reference order: (r0 + r1) + r2, then / 3
      const float sum = (to_f(ea[e]) + to_f(eb[e])) + to_f(ec[e]);
      eo[e] = from_f<T>(apply_act(sum * scale, act, slope));
    }
    __builtin_memcpy(y + i * EPV, eo, 16);
  }
}
int launch_avg3_act(int dtype, const void* a, const void* b, const void* c, void* y, int64_t n, float scale, int act,
                    float slope, hipStream_t s) {
  const int epv = dtype == DT_F32 ? 4 : 8;
  if (n % epv) TANGO_FAIL("avg3: n must be a multiple of the 16-byte vector");
  const int64_t nvec = n / epv;
  unsigned nb = (unsigned)((nvec + 255) / 256);
  if (nb > 8192) nb = 8192;
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((avg3_act_kernel<float>), dim3(nb), dim3(256), 0, s, (const float*)a, (const float*)b, (const float*)c, (float*)y, nvec, scale, act, slope); break;
    case DT_F16: hipLaunchKernelGGL((avg3_act_kernel<f16>), dim3(nb), dim3(256), 0, s, (const f16*)a, (const f16*)b, (const f16*)c, (f16*)y, nvec, scale, act, slope); break;
    case DT_BF16: hipLaunchKernelGGL((avg3_act_kernel<bf16>), dim3(nb), dim3(256), 0, s, (const bf16*)a, (const bf16*)b, (const bf16*)c, (bf16*)y, nvec, scale, act, slope); break;
    default: TANGO_FAIL("avg3: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

// encoder_attention_mask (bool) -> additive bias (1 - m) * -10000  (unet_2d_condition.py:575-579)
__global__ void mask_bias_kernel(const uint8_t* __restrict__ m, float* __restrict__ bias, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) bias[i] = (1.0f - (m[i] ? 1.0f : 0.0f)) * -10000.0f;
}
int launch_mask_bias(const uint8_t* mask, float* bias, int n, hipStream_t s) {
  hipLaunchKernelGGL(mask_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mask, bias, n);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// sinusoidal timestep embedding (models/embeddings.py:22-62), fp32 op-for-op
__global__ void timestep_embedding_kernel(const int64_t* __restrict__ ts, float* __restrict__ out, int n, int dim, int flip,
                                          float freq_shift) {
  const int i = blockIdx.x, half = dim / 2;
  for (int j = threadIdx.x; j < half; j += blockDim.x) {
    const float ex = __fdiv_rn(__fmul_rn(-9.210340371976184f, (float)j), (float)half - freq_shift);
    const float arg = __fmul_rn((float)ts[i], expf(ex));
    const float sv = sinf(arg), cv = cosf(arg);
    if (flip) { out[(int64_t)i * dim + j] = cv; out[(int64_t)i * dim + half + j] = sv; }
    else { out[(int64_t)i * dim + j] = sv; out[(int64_t)i * dim + half + j] = cv; }
  }
  if ((dim & 1) && threadIdx.x == 0) out[(int64_t)i * dim + dim - 1] = 0.f;
}
int launch_timestep_embedding(const int64_t* ts_dev, float* out, int n, int dim, int flip, float freq_shift, hipStream_t s) {
  hipLaunchKernelGGL(timestep_embedding_kernel, dim3((unsigned)n), dim3(256), 0, s, ts_dev, out, n, dim, flip, freq_shift);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------
// weight packing: dst[(row_off + rowmap(o)) * Kp + t*I + i] = src[o*so + t*st + i*si]; pad -> 0
// perm == 1: GEGLU row interleave (value row j -> 32*(j/16)+j%16, gate row j -> same + 16)
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int geglu_row(int o, int half) {
  const int j = o < half ? o : o - half;
  return 32 * (j >> 4) + (j & 15) + (o < half ? 0 : 16);
}

template <typename T>
__global__ __launch_bounds__(256) void pack_kernel(const float* __restrict__ src, T* __restrict__ dst, int O, int Tn, int I,
                                                   int64_t so, int64_t st, int64_t si, int64_t Kp, int64_t row_off, int perm) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)O * Kp) return;
  const int o = (int)(idx / Kp);
  const int k = (int)(idx - (int64_t)o * Kp);
  float v = 0.f;
  if (k < Tn * I) {
    const int t = k / I, i = k - t * I;
    v = src[(int64_t)o * so + (int64_t)t * st + (int64_t)i * si];
  }
  int orow = o;
  if (perm == 1) orow = geglu_row(o, O / 2);
  else if (perm == 2) orow = 32 * (o >> 4) + (o & 15);          // value half of a gated pair
  else if (perm == 3) orow = 32 * (o >> 4) + (o & 15) + 16;     // gate half
  dst[(row_off + orow) * Kp + k] = from_f<T>(v);
}

int launch_pack(int dtype, const float* src, void* dst, int O, int Tn, int I, int64_t so, int64_t st, int64_t si, int64_t Kp,
                int64_t dst_row_off, hipStream_t s) {
  const int perm = dst_row_off < 0 ? (int)(-dst_row_off) : 0;
  const int64_t ro = perm ? 0 : dst_row_off;
  const unsigned nb = (unsigned)(((int64_t)O * Kp + 255) / 256);
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((pack_kernel<float>), dim3(nb), dim3(256), 0, s, src, (float*)dst, O, Tn, I, so, st, si, Kp, ro, perm); break;
    case DT_F16: hipLaunchKernelGGL((pack_kernel<f16>), dim3(nb), dim3(256), 0, s, src, (f16*)dst, O, Tn, I, so, st, si, Kp, ro, perm); break;
    case DT_BF16: hipLaunchKernelGGL((pack_kernel<bf16>), dim3(nb), dim3(256), 0, s, src, (bf16*)dst, O, Tn, I, so, st, si, Kp, ro, perm); break;
    default: TANGO_FAIL("pack: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

// Phase weights of a nearest-x2 upsampler conv (conv_wide.hip PH; rule and layout: common.h launch_pack_ups_phase).  One thread per
// destination element; the up to four original taps are added in fp32 in ascending (ky, kx) order and rounded once.
template <typename T>
__global__ __launch_bounds__(256) void ups_phase_pack_kernel(const float* __restrict__ src, T* __restrict__ dst, int O, int I) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)16 * O * I) return;
  const int i = (int)(idx % I);
  const int tap = (int)((idx / I) & 3);
  const int o = (int)((idx / ((int64_t)4 * I)) % O);
  const int ph = (int)(idx / ((int64_t)4 * I * O));
  const int py = ph >> 1, px = ph & 1, ty = tap >> 1, tx = tap & 1;
  // rows(0, 0) = {0}, rows(0, 1) = {1, 2}, rows(1, 0) = {0, 1}, rows(1, 1) = {2}
  const int y0 = py ? (ty ? 2 : 0) : (ty ? 1 : 0), y1 = py ? (ty ? 2 : 1) : (ty ? 2 : 0);
  const int x0 = px ? (tx ? 2 : 0) : (tx ? 1 : 0), x1 = px ? (tx ? 2 : 1) : (tx ? 2 : 0);
  const float* w = src + ((int64_t)o * I + i) * 9;
  float v = 0.f;
  for (int ky = y0; ky <= y1; ++ky)
    for (int kx = x0; kx <= x1; ++kx) v += w[ky * 3 + kx];
  dst[idx] = from_f<T>(v);
}

int launch_pack_ups_phase(int dtype, const float* src, void* dst, int O, int I, hipStream_t s) {
  const unsigned nb = (unsigned)(((int64_t)16 * O * I + 255) / 256);
  switch (dtype) {
    case DT_F16: hipLaunchKernelGGL((ups_phase_pack_kernel<f16>), dim3(nb), dim3(256), 0, s, src, (f16*)dst, O, I); break;
    case DT_BF16: hipLaunchKernelGGL((ups_phase_pack_kernel<bf16>), dim3(nb), dim3(256), 0, s, src, (bf16*)dst, O, I); break;
    default: TANGO_FAIL("pack_ups_phase: 16-bit dtypes only");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}


// VAE: z * scale -> post_quant_conv (1x1, tiny C) fused with NCHW fp32 -> NHWC T
// (audioldm/variational_autoencoder/autoencoder.py:121 and :61)
template <typename T>
__global__ __launch_bounds__(256) void pointwise_small_kernel(const float* __restrict__ src, const float* __restrict__ W,
                                                              const float* __restrict__ bias, T* __restrict__ dst, int64_t ld,
                                                              int B, int Cin, int Cout, int HW, float scale) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * HW) return;
  const int b = (int)(idx / HW), hw = (int)(idx - (int64_t)b * HW);
  float x[16];
  for (int c = 0; c < Cin; ++c) x[c] = src[((int64_t)b * Cin + c) * HW + hw] * scale;
  for (int o = 0; o < Cout; ++o) {
    float a = bias ? bias[o] : 0.f;
    for (int c = 0; c < Cin; ++c) a += W[o * Cin + c] * x[c];
    dst[idx * ld + o] = from_f<T>(a);
  }
}
int launch_pointwise_small(int dtype, const float* src, const float* W, const float* b, void* dst, int64_t ld, int B, int Cin,
                           int Cout, int HW, float scale, hipStream_t s) {
  if (Cin > 16) TANGO_FAIL("pointwise_small: Cin > 16");
  const unsigned nb = (unsigned)(((int64_t)B * HW + 255) / 256);
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((pointwise_small_kernel<float>), dim3(nb), dim3(256), 0, s, src, W, b, (float*)dst, ld, B, Cin, Cout, HW, scale); break;
    case DT_F16: hipLaunchKernelGGL((pointwise_small_kernel<f16>), dim3(nb), dim3(256), 0, s, src, W, b, (f16*)dst, ld, B, Cin, Cout, HW, scale); break;
    case DT_BF16: hipLaunchKernelGGL((pointwise_small_kernel<bf16>), dim3(nb), dim3(256), 0, s, src, W, b, (bf16*)dst, ld, B, Cin, Cout, HW, scale); break;
    default: TANGO_FAIL("pointwise_small: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

// VAE encoder tail: moments = quant_conv(h) (autoencoder.py:56), 1x1 conv with tiny C on fp32 channels-last rows, written in
// the reference's NCHW fp32 layout
__global__ __launch_bounds__(256) void pointwise_out_nchw_kernel(const float* __restrict__ src, int64_t ld, const float* __restrict__ W,
                                                                 const float* __restrict__ bias, float* __restrict__ dst, int B, int Cin,
                                                                 int Cout, int HW) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * HW) return;
  const int b = (int)(idx / HW), hw = (int)(idx - (int64_t)b * HW);
  float x[32];
  for (int c = 0; c < Cin; ++c) x[c] = src[idx * ld + c];
  for (int o = 0; o < Cout; ++o) {
    float a = bias ? bias[o] : 0.f;
    for (int c = 0; c < Cin; ++c) a += W[o * Cin + c] * x[c];
    dst[((int64_t)b * Cout + o) * HW + hw] = a;
  }
}
int launch_pointwise_out_nchw(const float* src, int64_t ld, const float* W, const float* b, float* dst, int B, int Cin, int Cout, int HW,
                              hipStream_t s) {
  if (Cin > 32) TANGO_FAIL("pointwise_out_nchw: Cin > 32");
  const unsigned nb = (unsigned)(((int64_t)B * HW + 255) / 256);
  hipLaunchKernelGGL(pointwise_out_nchw_kernel, dim3(nb), dim3(256), 0, s, src, ld, W, b, dst, B, Cin, Cout, HW);
  TANGO_HIP(hipGetLastError());
  return 0;
}

__global__ void permute_geglu_bias_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[geglu_row(i, n / 2)] = src[i];
}
int launch_permute_geglu_bias(const float* src, float* dst, int n, hipStream_t s) {
  hipLaunchKernelGGL(permute_geglu_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, n);
  TANGO_HIP(hipGetLastError());
  return 0;
}

int launch_fill_zero(void* p, size_t bytes, hipStream_t s) {
  TANGO_HIP(hipMemsetAsync(p, 0, bytes, s));
  return 0;
}

// unused placeholder kept for ABI symmetry with common.h (time MLP runs through gemm<float>)
int launch_linear_f32(const float*, const float*, const float*, float*, int, int, int, int, int, hipStream_t) {
  TANGO_FAIL("linear_f32: not implemented (use launch_gemm with DT_F32)");
}

// ------------------------------------------------------------------------------------------
// Text encoder (FLAN-T5) helpers: embedding gather, T5LayerNorm, relative position bias
// (transformers models/t5/modeling_t5.py: T5LayerNorm, T5Attention.compute_bias; reference call site models.py:129-147)
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void embed_gather_kernel(const int64_t* __restrict__ ids, const float* __restrict__ table,
                                                           T* __restrict__ out, int64_t ld, int rows, int D, int vocab) {
  const int r = blockIdx.x;
  int64_t id = ids[r];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const float* src = table + id * D;
  T* dst = out + (int64_t)r * ld;
  for (int c = threadIdx.x * 4; c < D; c += 1024) {
    const f32x4 v = *(const f32x4*)(src + c);
    dst[c] = from_f<T>(v[0]); dst[c + 1] = from_f<T>(v[1]); dst[c + 2] = from_f<T>(v[2]); dst[c + 3] = from_f<T>(v[3]);
  }
}
int launch_embed_gather(int dtype, const int64_t* ids, const float* table, void* out, int64_t ld, int rows, int D, int vocab, hipStream_t s) {
  if (D % 4 != 0) TANGO_FAIL("embed_gather: d_model must be a multiple of 4");
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((embed_gather_kernel<float>), dim3((unsigned)rows), dim3(256), 0, s, ids, table, (float*)out, ld, rows, D, vocab); break;
    case DT_F16: hipLaunchKernelGGL((embed_gather_kernel<f16>), dim3((unsigned)rows), dim3(256), 0, s, ids, table, (f16*)out, ld, rows, D, vocab); break;
    case DT_BF16: hipLaunchKernelGGL((embed_gather_kernel<bf16>), dim3((unsigned)rows), dim3(256), 0, s, ids, table, (bf16*)out, ld, rows, D, vocab); break;
    default: TANGO_FAIL("embed_gather: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

// one wave per row; fp32 statistics (T5LayerNorm computes the variance in fp32 as well)
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const T* __restrict__ x, int64_t ldx, void* __restrict__ y, int64_t ldy,
                                                      const float* __restrict__ gamma, int rows, int C, float eps, int out_f32) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* xr = x + (int64_t)row * ldx;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) { const float f = to_f(xr[c]); q += f * f; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const float rstd = rsqrtf(q / (float)C + eps);
  for (int c = lane; c < C; c += 64) {
    const float v = to_f(xr[c]) * rstd * gamma[c];
    if (out_f32) ((float*)y)[(int64_t)row * ldy + c] = v;
    else ((T*)y)[(int64_t)row * ldy + c] = from_f<T>(v);
  }
}
int launch_rmsnorm(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, const float* gamma, int rows, int C, float eps, int out_f32,
                   hipStream_t s) {
  const unsigned nb = (unsigned)((rows + 3) / 4);
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((rmsnorm_kernel<float>), dim3(nb), dim3(256), 0, s, (const float*)x, ldx, y, ldy, gamma, rows, C, eps, out_f32); break;
    case DT_F16: hipLaunchKernelGGL((rmsnorm_kernel<f16>), dim3(nb), dim3(256), 0, s, (const f16*)x, ldx, y, ldy, gamma, rows, C, eps, out_f32); break;
    case DT_BF16: hipLaunchKernelGGL((rmsnorm_kernel<bf16>), dim3(nb), dim3(256), 0, s, (const bf16*)x, ldx, y, ldy, gamma, rows, C, eps, out_f32); break;
    default: TANGO_FAIL("rmsnorm: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

__global__ __launch_bounds__(256) void t5_pos_bias_kernel(const float* __restrict__ table, const int* __restrict__ bucket,
                                                          float* __restrict__ out, int heads, int L) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)heads * L * L) return;
  const int h = (int)(idx / ((int64_t)L * L));
  const int ij = (int)(idx - (int64_t)h * L * L);
  out[idx] = table[bucket[ij] * heads + h];
}
int launch_t5_pos_bias(const float* table, const int* bucket, float* out, int heads, int L, hipStream_t s) {
  const int64_t n = (int64_t)heads * L * L;
  hipLaunchKernelGGL(t5_pos_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, table, bucket, out, heads, L);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// ---- single-key cross-attention rows (round 4) -----------------------------------------------------------------------------
// A sample whose text mask keeps exactly ONE key (the unconditional rows of a CFG batch: T5("") padded, models.py:282-289) has
// softmax weights exactly (1, 0, ..., 0) under the reference's additive -10000 bias (exp underflows to 0 in fp32), so
//   attn2(norm2(x), text) + x  ==  to_out(v_key) + b_out + x
// for every query row: cvec is computed once per call (step-invariant), the per-step work is a broadcast add.
template <typename T>
__global__ __launch_bounds__(256) void xattn_const_kernel(const T* __restrict__ vt, int64_t ldvt, int C, const int* __restrict__ key0,
                                                          const T* __restrict__ wo, int64_t ldwo, const float* __restrict__ bo,
                                                          float* __restrict__ cvec) {
  const int b = blockIdx.x, n = blockIdx.y * 256 + threadIdx.x;
  if (n >= C) return;
  const T* v = vt + (int64_t)b * C * ldvt + key0[b];          // V^T [b][j][key]: stride ldvt over j
  const T* w = wo + (int64_t)n * ldwo;
  float acc = 0.f;
  for (int j = 0; j < C; ++j) acc = __builtin_fmaf(to_f(w[j]), to_f(v[(int64_t)j * ldvt]), acc);
  cvec[(int64_t)b * C + n] = acc + (bo ? bo[n] : 0.f);
}
int launch_xattn_const(int dtype, const void* vt, int64_t ldvt, int C, const int* key0, const void* wo, int64_t ldwo, const float* bo,
                       float* cvec, int nb, hipStream_t s) {
  if (nb <= 0) return 0;
  const dim3 grid((unsigned)nb, (unsigned)((C + 255) / 256));
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((xattn_const_kernel<float>), grid, dim3(256), 0, s, (const float*)vt, ldvt, C, key0, (const float*)wo, ldwo, bo, cvec); break;
    case DT_F16: hipLaunchKernelGGL((xattn_const_kernel<f16>), grid, dim3(256), 0, s, (const f16*)vt, ldvt, C, key0, (const f16*)wo, ldwo, bo, cvec); break;
    case DT_BF16: hipLaunchKernelGGL((xattn_const_kernel<bf16>), grid, dim3(256), 0, s, (const bf16*)vt, ldvt, C, key0, (const bf16*)wo, ldwo, bo, cvec); break;
    default: TANGO_FAIL("xattn_const: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

template <typename T>
__global__ __launch_bounds__(256) void rowbias_add_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ cvec, T* __restrict__ y,
                                                          int64_t ldy, int64_t rows, int rows_per, int C) {
  constexpr int V = 16 / (int)sizeof(T);                       // elements per 16-byte piece
  const int pieces = C / V;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * pieces) return;
  const int64_t r = idx / pieces;
  const int c0 = (int)(idx - r * pieces) * V;
  const float* cv = cvec + (r / rows_per) * C + c0;
  T in[V], out[V];
  __builtin_memcpy(in, x + r * ldx + c0, 16);
#pragma unroll
  for (int u = 0; u < V; ++u) out[u] = from_f<T>(to_f(in[u]) + cv[u]);
  __builtin_memcpy(y + r * ldy + c0, out, 16);
}
int launch_rowbias_add(int dtype, const void* x, int64_t ldx, const float* cvec, void* y, int64_t ldy, int64_t rows, int rows_per, int C,
                       hipStream_t s) {
  if (rows <= 0) return 0;
  const int esz = dtype == DT_F32 ? 4 : 2, V = 16 / esz;
  if (C % V != 0 || (ldx * esz) % 16 != 0 || (ldy * esz) % 16 != 0 || ((uintptr_t)x & 15) || ((uintptr_t)y & 15))
    TANGO_FAIL("rowbias_add: 16-byte alignment");
  const int64_t n = rows * (C / V);
  const unsigned grid = (unsigned)((n + 255) / 256);
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL((rowbias_add_kernel<float>), dim3(grid), dim3(256), 0, s, (const float*)x, ldx, cvec, (float*)y, ldy, rows, rows_per, C); break;
    case DT_F16: hipLaunchKernelGGL((rowbias_add_kernel<f16>), dim3(grid), dim3(256), 0, s, (const f16*)x, ldx, cvec, (f16*)y, ldy, rows, rows_per, C); break;
    case DT_BF16: hipLaunchKernelGGL((rowbias_add_kernel<bf16>), dim3(grid), dim3(256), 0, s, (const bf16*)x, ldx, cvec, (bf16*)y, ldy, rows, rows_per, C); break;
    default: TANGO_FAIL("rowbias_add: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

// y[r][0..C) = x[r][0..C) for strided row views (16-byte pieces); engine dtype irrelevant beyond its size
__global__ __launch_bounds__(256) void copy_rows_kernel(const unsigned char* __restrict__ x, int64_t ldx_b, unsigned char* __restrict__ y, int64_t ldy_b,
                                                        int64_t rows, int pieces) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * pieces) return;
  const int64_t r = idx / pieces;
  const int pc = (int)(idx - r * pieces);
  *(u32x4*)(y + r * ldy_b + (int64_t)pc * 16) = *(const u32x4*)(x + r * ldx_b + (int64_t)pc * 16);
}
int launch_copy_rows(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int C, hipStream_t s) {
  if (rows <= 0) return 0;
  const int esz = dtype == DT_F32 ? 4 : 2;
  if ((C * esz) % 16 != 0 || (ldx * esz) % 16 != 0 || (ldy * esz) % 16 != 0 || ((uintptr_t)x & 15) || ((uintptr_t)y & 15))
    TANGO_FAIL("copy_rows: 16-byte alignment");
  const int pieces = C * esz / 16;
  const int64_t n = rows * pieces;
  hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const unsigned char*)x, ldx * esz, (unsigned char*)y,
                     ldy * esz, rows, pieces);
  TANGO_HIP(hipGetLastError());
  return 0;
}

}  // namespace tango

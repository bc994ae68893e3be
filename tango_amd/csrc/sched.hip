// The denoise loop's own kernels (fused CFG combine + scheduler update for DDPM / DDIM and multistep DPM-Solver with its masked and guided
// variants, guidance statistics, inpainting blend, step counter, Philox, fused latent encode, the windowed update of long clips and of loops
// with their gathers, the mel tile blends and the vocoder's ring padding), their launchers and their argument checkers.
#include <cmath>
#include "common.h"
#include "tango_engine.h"

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

// ------------------------------------------------------------------------------------------
// Long clips: MultiDiffusion (Bar-Tal et al. 2023) windows in time, fused into the update.  The fork's panorama pipeline
// (mustango/diffusers/src/diffusers/pipelines/stable_diffusion/pipeline_stable_diffusion_panorama.py:442-456 get_views, :614-652 the
// per-step loop value += step(view); count += 1; latents = value / count) steps every view on its own and averages.  Here the views
// of a clip are rows of one UNet batch (common.h WindowGeom) and this kernel closes the step: one thread per CANVAS position
// (b, h, w), per channel
//   d_v = sched_step_kernel's `prev` before its sig * nz term, from rows (b, v) of eps at window position (h - v s, w)   v in cover(h), ascending
//   acc = 0; acc = acc + d_v;   r = acc / |cover(h)|   (IEEE division);   if sig > 0: r = r + sig * nz
// with the same fp32 operations in the same order (no FMA contraction).  r goes to the canvas and, as T, to every window row of the
// next UNet input that covers h, in both CFG halves.  V = 1: (0 + d) / 1 is exact, the step is sched_step_kernel's bit for bit.
// Two deliberate deviations from the fork: (1) the views must cover the canvas exactly ((H - Hw) % s == 0 is the caller's to meet; get_views
// floors and leaves a tail of rows with count == 0); (2) nz is ONE draw per canvas element -- injected noise[step][b, c, h, w] or Philox with
// the canvas position as the counter's hw -- where the fork's loop would average V independent draws and shrink the variance of a
// stochastic sampler's step noise by |cover(h)|.  With sig == 0 (DDIM eta = 0, the last DDPM step) it is the fork's loop.
// g.ring (loops, tango_engine_denoise_ring): the canvas rows are a ring and the views wrap round it.  The mode is data of the block: it
// changes only the three integers of the cover (common.h window_cover), computed once per thread; both modes then walk the views
// (v0 + j) mod V at local rows y0 - j s with the same per-view arithmetic.  On a ring the view that starts farthest below h comes first
// -- for a row that no view wraps over, the ascending order above.  The order is relative to h, so the update commutes with a rotation
// of the ring by a multiple of s: no row is special, the wrap point included.
// WEIGHTED (timed prompts, tango_engine_denoise_*_weighted): weighted MultiDiffusion / "Mixture of Diffusers" (Jimenez 2023).  The block's
// `weights` is a device table of Hw positive floats, one per local window row, shared by all views; over the same views in the same order
//   acc = 0; wsum = 0;   t = w[y_v] * d_v; acc = acc + t; wsum = wsum + w[y_v];   r = acc / wsum   (IEEE division);   + sig * nz as above
// so a view fades in and out over its overlaps instead of counting in full up to its last row.  wsum does not depend on the channel and is
// summed once per thread.  All weights 1: t = d and wsum = n are exact, the unweighted kernel's bits.  One view with w != 1: (w d) / w may
// differ from d in the last bit; there is no special case.
// ------------------------------------------------------------------------------------------
template <typename T, bool WEIGHTED>
__global__ __launch_bounds__(256) void sched_window_kernel(const SchedWindowParams* __restrict__ pp) {
#pragma clang fp contract(off)
  const SchedParams p = pp->p;
  const WindowGeom g = pp->g;
  const int W = pp->W, noise_row0 = pp->noise_row0;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.B * p.HW) return;
  const int b = idx / p.HW, hw = idx - b * p.HW;
  const int h = hw / W, w = hw - h * W;
  int v0, y0;                                       // the cover: n views from v0 at local row y0, then one view up and s rows down
  const int n = window_cover(g, h, &v0, &y0);
  float cnt = (float)n;
  const float* wt = nullptr;
  if constexpr (WEIGHTED) {
    wt = pp->weights;
    cnt = 0.0f;
    for (int j = 0, y = y0; j < n; ++j, y -= g.s) cnt = cnt + wt[y];
  }
  const int step = *p.step_ptr;
  const float* cf = p.coef + step * 8;
  const float sa = cf[0], sb = cf[1], c0 = cf[2], c1 = cf[3], sig = cf[4], sap = cf[5], dirc = cf[6];
  const int C = p.C;
  const int64_t win = (int64_t)g.Hw * W;            // positions of one window
  const int64_t half = (int64_t)p.B * g.V * win;    // positions of one CFG half of the window batch
  float nrm[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    float* lp = p.lat + ((int64_t)b * C + c) * p.HW + hw;
    const float x = *lp;
    float acc = 0.0f;
    for (int j = 0, v = v0, y = y0; j < n; ++j, y -= g.s) {
      const int64_t pos = ((int64_t)b * g.V + v) * win + (int64_t)y * W + w;
      if (++v == g.V) v = 0;                          // (only a ring's views wrap)
      float o = p.eps[pos * C + c];
      if (p.cfg) { const float dlt = p.eps[(half + pos) * C + c] - o; const float gd = p.guidance * dlt; o = o + gd; }   // models.py:246
      float x0;
      if (p.pred_type == 0) { const float m0 = sb * o; const float d0 = x - m0; x0 = d0 / sa; }   // epsilon
      else if (p.pred_type == 1) x0 = o;                                                          // sample
      else { const float m0 = sa * x; const float m1 = sb * o; x0 = m0 - m1; }                    // v_prediction
      if (p.clip) x0 = fminf(fmaxf(x0, -p.clip_range), p.clip_range);
      float d;
      if (p.rule == 0) {
        const float m0 = c0 * x0; const float m1 = c1 * x; d = m0 + m1;
      } else {
        float e;
        if (p.pred_type == 0) e = o;
        else if (p.pred_type == 1) { const float m0 = sa * x0; const float d0 = x - m0; e = d0 / sb; }
        else { const float m0 = sa * o; const float m1 = sb * x; e = m0 + m1; }
        const float m0 = sap * x0; const float m1 = dirc * e; d = m0 + m1;
      }
      if constexpr (WEIGHTED) d = wt[y] * d;
      acc = acc + d;
    }
    float r = acc / cnt;
    if (sig > 0.f) {
      float nz;
      if (p.noise) {
        nz = p.noise[(int64_t)(step - noise_row0) * p.B * C * p.HW + ((int64_t)b * C + c) * p.HW + hw];
      } else {
        if ((c & 3) == 0) philox_normal4(hw, c >> 2, p.sample_offset + b, step, p.seed, nrm);   // one draw per 4 channels
        nz = nrm[c & 3];
      }
      const float m2 = sig * nz; r = r + m2;
    }
    *lp = r;
    const T tv = from_f<T>(r);
    for (int j = 0, v = v0, y = y0; j < n; ++j, y -= g.s) {
      const int64_t pos = ((int64_t)b * g.V + v) * win + (int64_t)y * W + w;
      if (++v == g.V) v = 0;
      ((T*)p.xin)[pos * p.xin_ld + c] = tv;
      if (p.cfg) ((T*)p.xin)[(half + pos) * p.xin_ld + c] = tv;
    }
  }
}

// canvas fp32 NCHW -> the window batch T NHWC before step 0: the windowed form of nchw_to_nhwc_kernel with rep CFG halves.  One
// thread per (window row, position); a canvas element that V' views cover is read V' times.  Window position (y, w) of view v is
// canvas position (v s + y, w), minus H rows when v s + y reaches H: only a ring's views get there, and v s + y < H + Hw <= 2 H.
template <typename T>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ lat, T* __restrict__ xin, int64_t ld, int B, int C, int W,
                                                            WindowGeom g, int rep) {
  const int64_t win = (int64_t)g.Hw * W;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * g.V * win) return;
  const int row = (int)(idx / win), pos = (int)(idx - (int64_t)row * win);
  const int b = row / g.V, v = row - b * g.V;
  const int64_t HW = (int64_t)g.H * W;
  int64_t src = (int64_t)v * g.s * W + pos;             // (v s + y) W + w
  if (src >= HW) src -= HW;                             // v s + y >= H: the view wraps
  for (int c = 0; c < C; ++c) {
    const T t = from_f<T>(lat[((int64_t)b * C + c) * HW + src]);
    for (int r = 0; r < rep; ++r) xin[((int64_t)r * B * g.V * win + idx) * ld + c] = t;
  }
}

// the same gather fp32 NCHW -> fp32 NCHW [B * V, C, Hw, W] (the input of the tiled VAE decode): one thread per output element
__global__ __launch_bounds__(256) void window_gather_nchw_kernel(const float* __restrict__ lat, float* __restrict__ dst, int B, int C, int W,
                                                                 WindowGeom g) {
  const int64_t win = (int64_t)g.Hw * W;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * g.V * C * win) return;
  const int64_t rc = idx / win;                          // (b V + v) C + c
  const int pos = (int)(idx - rc * win);
  const int c = (int)(rc % C), row = (int)(rc / C);
  const int b = row / g.V, v = row - b * g.V;
  const int64_t HW = (int64_t)g.H * W;
  int64_t src = (int64_t)v * g.s * W + pos;
  if (src >= HW) src -= HW;
  dst[idx] = lat[((int64_t)b * C + c) * HW + src];
}

// Cross-fade of the V decoded tiles of a clip (the fork's tiled VAE decode, mustango/diffusers/src/diffusers/models/autoencoder_kl.py
// :198-201 blend_v, :255-296).  g counts mel rows: tile t holds output rows t s + y for y in [0, Hw) (mod H on a ring), E = Hw - s rows
// overlap.  The weight of tile t at its local row y is min(1, (y + 0.5) / E) if it has a predecessor (t > 0, or a ring), times
// min(1, (Hw - y - 0.5) / E) if it has a successor (t < V - 1, or a ring); both 1 when E == 0.  Then
//   out[r] = (sum_t w_t tile_t) / (sum_t w_t)   over the covering tiles in window_cover's order, each sum from 0, in fp32 without FMA contraction.
// For s >= Hw / 2 two overlapping weights sum to 1: blend_v's linear ramp sampled at half-pixel centres; deeper overlaps use the same formula.
__global__ __launch_bounds__(256) void mel_tile_blend_kernel(const float* __restrict__ tiles, float* __restrict__ out, int B, int F, WindowGeom g) {
#pragma clang fp contract(off)
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * g.H * F) return;
  const int f = (int)(idx % F);
  const int64_t br = idx / F;
  const int r = (int)(br % g.H), b = (int)(br / g.H);
  int t, y;
  const int n = window_cover(g, r, &t, &y);
  const int E = g.Hw - g.s;
  float num = 0.0f, den = 0.0f;
  for (int j = 0; j < n; ++j, y -= g.s) {
    float wt = 1.0f;
    if (E > 0 && (g.ring || t > 0)) { const float a = (float)y + 0.5f; wt = fminf(1.0f, a / (float)E); }
    if (E > 0 && (g.ring || t < g.V - 1)) { const float a = (float)(g.Hw - y) - 0.5f; const float u = fminf(1.0f, a / (float)E); wt = wt * u; }
    const float m = wt * tiles[(((int64_t)b * g.V + t) * g.Hw + y) * F + f];
    if (++t == g.V) t = 0;                              // (only a ring's tiles wrap)
    num = num + m;
    den = den + wt;
  }
  out[idx] = num / den;
}

// the vocoder's context on a ring: dst frame j of [T + 2 ctx] is mel frame (j - ctx) mod T (ctx may exceed T: the ring is walked more than once)
__global__ __launch_bounds__(256) void mel_ring_pad_kernel(const float* __restrict__ mel, float* __restrict__ dst, int B, int T, int F, int ctx) {
  const int Tp = T + 2 * ctx;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)B * Tp * F) return;
  const int f = (int)(idx % F);
  const int64_t bj = idx / F;
  const int j = (int)(bj % Tp), b = (int)(bj / Tp);
  int t = (j - ctx) % T;
  if (t < 0) t += T;
  dst[idx] = mel[((int64_t)b * T + t) * F + f];
}

int launch_mel_ring_pad(const float* mel, float* dst, int B, int T, int F, int ctx, hipStream_t s) {
  if (B <= 0 || T <= 0 || F <= 0 || ctx < 0) TANGO_FAIL("mel_ring_pad: bad sizes");
  const dim3 grid((unsigned)(((int64_t)B * (T + 2 * ctx) * F + 255) / 256));
  hipLaunchKernelGGL(mel_ring_pad_kernel, grid, dim3(256), 0, s, mel, dst, B, T, F, ctx);
  TANGO_HIP(hipGetLastError());
  return 0;
}

int launch_window_gather(int dtype, const float* lat, void* xin, int64_t ld, int B, int C, int W, const WindowGeom& g, int rep, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)B * g.V * g.Hw * W + 255) / 256));
  switch (dtype) {
    case DT_F32: hipLaunchKernelGGL(window_gather_kernel<float>, grid, dim3(256), 0, s, lat, (float*)xin, ld, B, C, W, g, rep); break;
    case DT_F16: hipLaunchKernelGGL(window_gather_kernel<f16>, grid, dim3(256), 0, s, lat, (f16*)xin, ld, B, C, W, g, rep); break;
    case DT_BF16: hipLaunchKernelGGL(window_gather_kernel<bf16>, grid, dim3(256), 0, s, lat, (bf16*)xin, ld, B, C, W, g, rep); break;
    default: TANGO_FAIL("window_gather: bad dtype");
  }
  TANGO_HIP(hipGetLastError());
  return 0;
}

int launch_window_gather_nchw(const float* lat, float* dst, int B, int C, int W, const WindowGeom& g, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)B * g.V * C * g.Hw * W + 255) / 256));
  hipLaunchKernelGGL(window_gather_nchw_kernel, grid, dim3(256), 0, s, lat, dst, B, C, W, g);
  TANGO_HIP(hipGetLastError());
  return 0;
}

int launch_mel_tile_blend(const float* tiles, float* out, int B, int F, const WindowGeom& g, hipStream_t s) {
  const dim3 grid((unsigned)(((int64_t)B * g.H * F + 255) / 256));
  hipLaunchKernelGGL(mel_tile_blend_kernel, grid, dim3(256), 0, s, tiles, out, B, F, g);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// One message per condition; a ring's are H >= Hw, H % s == 0, 1 <= s <= Hw, V = H / s <= kMaxWindows, asked in that order.
const char* window_geom_refusal(int canvas_h, int window_h, int stride, bool ring, WindowGeom* g) {
  if (window_h <= 0) return "window_h must be positive";
  int V;
  if (ring) {
    if (canvas_h < window_h) return "the ring must be at least window_h rows long";
    if (stride >= 1 && canvas_h % stride != 0) return "the ring's height must be a multiple of stride";
    if (stride < 1 || stride > window_h) return "stride must be in [1, window_h]";
    V = canvas_h / stride;
  } else {
    if (stride < 1 || stride > window_h) return "stride must be in [1, window_h]";
    if (canvas_h < window_h) return "the canvas height must be at least window_h";
    if ((canvas_h - window_h) % stride != 0)
      return "the windows must cover the canvas exactly: (canvas height - window_h) must be a multiple of stride";
    V = (canvas_h - window_h) / stride + 1;
  }
  if (V > kMaxWindows) return ring ? "at most 32 windows per ring" : "at most 32 windows per clip";
  if (g) { g->H = canvas_h; g->Hw = window_h; g->s = stride; g->V = V; g->ring = ring; }
  return nullptr;
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

// Every instantiation of the update kernels, spelled once: [multistep][masked][guided][dtype] (dtype in DType's order)
typedef void (*SchedKernel)(const SchedParams*);
#define TANGO_SCHED_DTYPES(K, ...) {K<float, ##__VA_ARGS__>, K<f16, ##__VA_ARGS__>, K<bf16, ##__VA_ARGS__>}
static const SchedKernel kSchedKernels[2][2][2][3] = {
    {{TANGO_SCHED_DTYPES(sched_step_kernel, false, false), TANGO_SCHED_DTYPES(sched_step_kernel, false, true)},
     {TANGO_SCHED_DTYPES(sched_step_kernel, true, false), TANGO_SCHED_DTYPES(sched_step_kernel, true, true)}},
    {{TANGO_SCHED_DTYPES(sched_multistep_kernel, false, false), TANGO_SCHED_DTYPES(sched_multistep_kernel, false, true)},
     {TANGO_SCHED_DTYPES(sched_multistep_kernel, true, false), TANGO_SCHED_DTYPES(sched_multistep_kernel, true, true)}}};
static const SchedKernel kBlend0Kernels[3] = TANGO_SCHED_DTYPES(inpaint_blend0_kernel);
typedef void (*SchedWindowKernel)(const SchedWindowParams*);
static const SchedWindowKernel kSchedWindowKernels[2][3] = {TANGO_SCHED_DTYPES(sched_window_kernel, false),   // [weighted][dtype]
                                                            TANGO_SCHED_DTYPES(sched_window_kernel, true)};
#undef TANGO_SCHED_DTYPES

// one thread per latent position: the grid covers max_positions >= B * HW of the block, surplus threads exit
static int launch_sched_kernel(SchedKernel k, const SchedParams* dev_params, int max_positions, hipStream_t s) {
  hipLaunchKernelGGL(k, dim3((unsigned)((max_positions + 255) / 256)), dim3(256), 0, s, dev_params);
  TANGO_HIP(hipGetLastError());
  return 0;
}

int launch_inpaint_blend0(int dtype, const SchedParams* dev_params, int max_positions, hipStream_t s) {
  if (dtype < DT_F32 || dtype > DT_BF16) TANGO_FAIL("inpaint_blend0: bad dtype");
  return launch_sched_kernel(kBlend0Kernels[dtype], dev_params, max_positions, s);
}

int launch_sched_step(int dtype, const SchedParams* dev_params, int max_positions, hipStream_t s, int rule, bool masked, bool guided) {
  if (dtype < DT_F32 || dtype > DT_BF16) TANGO_FAIL("sched_step: bad dtype");
  return launch_sched_kernel(kSchedKernels[rule == TANGO_RULE_DPM_MULTISTEP][masked][guided][dtype], dev_params, max_positions, s);
}

int launch_sched_window(int dtype, const SchedWindowParams* dev_params, int max_positions, bool weighted, hipStream_t s) {
  if (dtype < DT_F32 || dtype > DT_BF16) TANGO_FAIL("sched_window: bad dtype");
  hipLaunchKernelGGL(kSchedWindowKernels[weighted][dtype], dim3((unsigned)((max_positions + 255) / 256)), dim3(256), 0, s, dev_params);
  TANGO_HIP(hipGetLastError());
  return 0;
}

__global__ void step_inc_kernel(int* sp) { if (threadIdx.x == 0 && blockIdx.x == 0) *sp = *sp + 1; }
int launch_step_inc(int* step_ptr, hipStream_t s) {
  hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(64), 0, s, step_ptr);
  TANGO_HIP(hipGetLastError());
  return 0;
}

// Why the update step refuses these arguments (nullptr: it does not).  Host only: reads the coefficient rows [row0, row1) and the
// guidance rows it is given, nothing else.  The engine's callers read these messages: wording and order are pinned by tests.
const char* sched_args_refusal(const SchedArgs& a) {
  if (a.num_rows <= 0) return "num_steps must be positive";
  if (a.rule != TANGO_RULE_DDPM && a.rule != TANGO_RULE_DDIM && a.rule != TANGO_RULE_DPM_MULTISTEP) return "unknown rule";
  const bool ms = a.rule == TANGO_RULE_DPM_MULTISTEP;
  if (a.coef_w != (ms ? 16 : 8)) return ms ? "the multistep rule takes 16-float coefficient rows (coef_width 16)"
                                           : "DDPM / DDIM take 8-float coefficient rows (coef_width 0 or 8)";
  if (ms && a.noise) return "the multistep rule is deterministic: noise must be NULL";
  if (ms && a.clip) return "clip_sample is not supported by the multistep rule";
  if (ms && a.coef[11] != 0.0f && a.coef[11] != 1.0f) return "multistep table column 11 (algorithm) must be 0 or 1";
  if (ms) {
    for (int i = a.row0; i < a.row1; ++i) {          // a row never reads a history slot this loop has not written
      const float o = a.coef[(size_t)i * 16 + 10];
      if (!(o == 1.0f || (o == 2.0f && i >= 1) || (o == 3.0f && i >= 2))) return "multistep table row with a bad order";
    }
  }
  const bool mk = a.known != nullptr;
  if (mk != (a.mask != nullptr)) return "known_latents and latent_mask go together";
  if (mk && !a.blend_coef) return "a masked call needs blend_coef [num_steps][2]";
  if (!mk && (a.blend_coef || a.blend_noise)) return "blend_coef / blend_noise need known_latents and latent_mask";
  if (!a.guided) return nullptr;
  if (!(a.rescale >= 0.0f && a.rescale <= 1.0f)) return "guidance rescale must be in [0, 1]";
  if (a.rescale > 0.0f && !a.cfg_on) return "guidance rescale needs classifier-free guidance (guidance_scale > 1 or a guidance table)";
  if (a.table) {
    if (a.batch <= 0) return "a guidance table needs batch > 0";
    const size_t n = (size_t)a.table_rows * (size_t)a.batch;
    for (size_t i = 0; i < n; ++i)
      if (!(a.table[i] >= 0.0f) || std::isinf(a.table[i])) return "guidance table entries must be finite and >= 0";
  }
  return nullptr;
}

// Why the windowed update refuses these arguments, in this order: the multistep rule, what the plain update refuses, what else windows leave
// out, the geometry.  A ring says "on a ring" where a linear canvas says "with windows".
const char* window_args_refusal(const SchedArgs& a, int canvas_h, int window_h, int stride, bool ring, WindowGeom* g) {
  if (a.rule == TANGO_RULE_DPM_MULTISTEP)           // first: whatever its table looks like
    return ring ? "the multistep rule is not supported on a ring: use DDPM or DDIM"
                : "the multistep rule is not supported with windows (a per-view history has no reference behaviour): use DDPM or DDIM";
  if (const char* why = sched_args_refusal(a)) return why;
  if (a.known) return ring ? "known_latents (masked-latent inpainting) is not supported on a ring"
                           : "known_latents (masked-latent inpainting) is not supported with windows";
  if (a.guided && (a.table || a.rescale > 0.0f)) return ring ? "a guidance table or rescale is not supported on a ring"
                                                             : "a guidance table or rescale is not supported with windows";
  if (canvas_h <= 0) return ring ? "a ring call states its canvas height (latent_h > 0)" : "a windowed call states its canvas height (latent_h > 0)";
  if (const char* why = window_geom_refusal(canvas_h, window_h, stride, ring, g)) return why;
  if (window_h % 8 != 0) return "window_h is not a UNet height";
  return nullptr;
}

// Why a weighted update refuses its table (HOST [window_h]); asked after the unweighted call's own refusals.  The engine takes any
// positive table; the taper of timed prompts is tango_amd/inpaint.py window_taper.
const char* view_weights_refusal(const float* weights, int window_h) {
  if (!weights) return "view_weights must not be NULL (the unweighted call takes no table)";
  for (int y = 0; y < window_h; ++y)
    if (!(weights[y] > 0.0f) || std::isinf(weights[y])) return "view_weights entries must be finite and > 0";
  return nullptr;
}

}  // namespace tango

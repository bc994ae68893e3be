// HBM-bound elementwise / layout / packing kernels of the Tango engine.
#include "common.h"

namespace tango {

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

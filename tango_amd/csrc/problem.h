// The geometry of every GEMM-shaped problem, stated once (host only; included at the end of common.h).  The engine's plan builders, the
// per-op test wrappers (ops_abi.hip) and the host-only route queries (tango_debug_*_route) all build their GemmParams here, so a query
// answers for exactly the problem a wrapper launches and a plan records.  The constructors fill shapes and dense strides; the caller
// sets the pointers (with lda / Kp / ldo where its buffers are pitched) and the epilogue fields.
#pragma once
#include "common.h"

namespace tango {

// a dense (no gather) problem out[M, N] = A[M, K] @ W[N, K]^T with row strides lda / Kp
inline GemmParams dense_gemm(const void* A, int64_t lda, const void* W, int64_t Kp, int M, int N, int K) {
  GemmParams p;
  p.A = A; p.lda = lda; p.W = W; p.Kp = Kp;
  p.M = M; p.N = N; p.K = K; p.Cin = K;
  p.mode = GATHER_1D; p.rows_pb = M; p.Lin = M; p.Lout = M; p.taps = 1;
  return p;
}

// this GATHER_1D problem is a plain linear: row m of A is row m of the source, row m of the output is row m of `out`, and every row exists
// (Lin >= M; a shorter source needs the gather's zero fill, i.e. the conv1d form).  What dense_gemm() builds; of the constructors below only
// conv1d_problem with k = 1, B = 1 and a one-tap, stride-1, unpadded transposed-conv phase also qualify, and both have Lin == M.
inline bool gemm_is_plain_linear(const GemmParams& p) {
  return p.mode == GATHER_1D && p.taps == 1 && p.rows_pb == p.M && p.in_mul == 1 && p.in_off == 0 && p.out_mul == 1 && p.out_off == 0 &&
         p.Lin >= p.M;
}

inline int conv_out_dim(int n, int stride, int pad) { return (n + pad + 1 - 3) / stride + 1; }   // pad 1: symmetric; pad 0: zero row / column at the far edge only

// 3x3 gather conv on NHWC (Cin * esz a multiple of 64 bytes); H, W are the SOURCE dims (nearest-upsampled x2 first when `upsample`)
inline GemmParams conv2d_problem(int B, int Cin, int H, int W, int Cout, int stride, int upsample, int pad) {
  const int Hc = H << upsample, Wc = W << upsample;
  const int Ho = conv_out_dim(Hc, stride, pad), Wo = conv_out_dim(Wc, stride, pad);
  GemmParams p;
  p.N = Cout; p.ldo = Cout;
  p.lda = Cin; p.Kp = 9 * (int64_t)Cin; p.M = B * Ho * Wo; p.K = 9 * Cin; p.Cin = Cin;
  p.mode = GATHER_2D; p.H = Ho; p.Wd = Wo; p.Hin = H; p.Win = W; p.stride = stride; p.ups = upsample; p.pad = pad;
  return p;
}
// the same conv for tiny Cin: im2col rows [B*H*W][Kp] and a plain GEMM (stride 1, pad 1 only)
inline GemmParams conv2d_im2col_problem(int B, int Cin, int H, int W, int Cout) {
  const int64_t Kp = ((9 * Cin + 31) / 32) * 32;
  GemmParams p = dense_gemm(nullptr, Kp, nullptr, Kp, B * H * W, Cout, (int)Kp);
  p.ldo = Cout;
  return p;
}
// conv1d taps / transposed-conv1d phase taps on channels-last [B][Lin][Cin]: row q of a batch item reads q + in_off + tap * tap_step
// and writes row q * out_mul + out_off of [B][Lout][Cout]
inline GemmParams gather1d_problem(int B, int Cin, int Lin, int Cout, int taps, int tap_step, int in_off, int rows_pb, int Lout, int out_mul,
                                   int out_off) {
  GemmParams p;
  p.lda = Cin; p.Kp = (int64_t)taps * Cin; p.M = B * rows_pb; p.N = Cout; p.K = taps * Cin; p.Cin = Cin;
  p.mode = GATHER_1D; p.rows_pb = rows_pb; p.Lin = Lin; p.taps = taps; p.tap_step = tap_step; p.in_off = in_off;
  p.Lout = Lout; p.out_mul = out_mul; p.out_off = out_off; p.ldo = Cout;
  return p;
}
inline GemmParams conv1d_problem(int B, int Cin, int L, int Cout, int k, int dilation) {
  return gather1d_problem(B, Cin, L, Cout, k, dilation, -dilation * (k - 1) / 2, L, L, 1, 0);
}
// phase r of ConvTranspose1d(k, stride u, padding pd): outputs t = u * q + r - pd read inputs q - tap; false: the phase has no taps or no rows
inline bool convt_phase_problem(int B, int Cin, int L, int Cout, int k, int u, int pd, int r, GemmParams& p) {
  const int Lo = (L - 1) * u - 2 * pd + k;
  const int T = (k - r + u - 1) / u;
  if (T <= 0) return false;
  const int qmin = (pd > r) ? (pd - r + u - 1) / u : 0;
  const int qmax = (Lo - 1 + pd - r) / u;
  const int Q = qmax - qmin + 1;
  if (Q <= 0) return false;
  p = gather1d_problem(B, Cin, L, Cout, T, -1, qmin, Q, Lo, u, u * qmin + r - pd);
  return true;
}

}  // namespace tango

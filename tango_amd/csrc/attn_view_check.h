// What tango_op_attention_view (ops_abi.hip) refuses before it launches anything: one pure host function of its arguments and the four
// base addresses it staged, with no HIP in it, so that tools/attn_view_check_main.cpp can run it stand-alone under ASan + UBSan.
// Everything that could take attn_kernel outside the staged buffers ends here: the kernel reads Q, K and V^T in 16-byte pieces at
// 32-bit per-thread offsets (row * ld), stores O in 8-byte pieces (16 in the LDS-staged form) and multiplies the V^T columns >= Skv
// by an exact-zero weight (AttnParams: "zero / finite").
#pragma once
#include <cmath>
#include <cstdint>

namespace tango {

struct AttnViewArgs {
  int dtype = 0;                        // 0 fp32, 1 fp16, 2 bf16
  int B = 0, heads = 0, Sq = 0, Skv = 0;
  int flags = 0;                        // as tango_op_attention_ex: 1 fp8 P.V, 2 (with 1) the MX form, 4 v rows in fragment order
  bool bias = false, pos_bias = false;
  int64_t ldq = 0, ldk = 0, k_col0 = -1, ldvt = 0, ldo = 0, o_col0 = 0;
  float pad_value = 0.0f;
  uintptr_t q_base = 0, k_base = 0, vt_base = 0, o_base = 0;   // what AttnParams::q / k / vt / o will hold
};

static constexpr int64_t kAttnViewMaxLd = 65536;          // row * ld * sizeof(T) stays far inside the kernel's 32-bit offsets
static constexpr int64_t kAttnViewMaxElems = 1ll << 28;   // per staged buffer (the staging launches count rows in an int)

// the refusal's message, or null
inline const char* attn_view_refusal(const AttnViewArgs& a) {
  if (a.dtype < 0 || a.dtype > 2) return "op_attention_view: bad dtype";
  if (a.B <= 0 || a.heads <= 0 || a.Sq <= 0 || a.Skv <= 0) return "op_attention_view: bad sizes";
  if (!std::isfinite(a.pad_value)) return "op_attention_view: pad_value must be finite (V^T columns >= Skv are multiplied by a zero weight)";
  const int64_t esz = a.dtype == 0 ? 4 : 2;
  const int64_t C = (int64_t)a.heads * 64;
  const int64_t ldvt_min = ((int64_t)a.Skv + 7) / 8 * 8;
  if (a.ldq < C || a.ldk < C || a.ldo < C) return "op_attention_view: ldq, ldk and ldo must be at least heads * 64";
  if (a.ldvt < ldvt_min) return "op_attention_view: ldvt must be at least round8(Skv)";
  if (a.ldq > kAttnViewMaxLd || a.ldk > kAttnViewMaxLd || a.ldvt > kAttnViewMaxLd || a.ldo > kAttnViewMaxLd)
    return "op_attention_view: a pitch beyond 65536 elements";
  if (a.k_col0 < -1) return "op_attention_view: k_col0 is a column of the shared buffer or -1";
  if (a.k_col0 >= 0) {
    if (a.Sq != a.Skv || a.ldk != a.ldq) return "op_attention_view: k_col0 >= 0 (one buffer for q | k) needs Sq == Skv and ldk == ldq";
    if (a.k_col0 < C) return "op_attention_view: k_col0 inside the columns of q";
    if (a.k_col0 + C > a.ldq) return "op_attention_view: k_col0 + heads * 64 exceeds ldq";
  }
  if (a.o_col0 < 0) return "op_attention_view: o_col0 is negative";
  if (a.o_col0 + C > a.ldo) return "op_attention_view: o_col0 + heads * 64 exceeds ldo";
  const int64_t rows_q = (int64_t)a.B * a.Sq, rows_k = (int64_t)a.B * a.Skv;
  if (rows_q * a.ldq > kAttnViewMaxElems || rows_k * a.ldk > kAttnViewMaxElems || (int64_t)a.B * C * a.ldvt > kAttnViewMaxElems ||
      rows_q * a.ldo > kAttnViewMaxElems || (int64_t)a.heads * a.Sq > kAttnViewMaxElems / a.Skv)     // the last: pos_bias [heads][Sq][Skv]
    return "op_attention_view: problem too large for a test hook";
  if (a.q_base % 16 || a.k_base % 16 || a.vt_base % 16) return "op_attention_view: the q, k and v^T bases must be 16-byte aligned (k_col0 is in elements)";
  if (a.o_base % 8) return "op_attention_view: the output base must be 8-byte aligned (o_col0 is in elements)";
  if ((a.ldq * esz) % 16 || (a.ldk * esz) % 16 || (a.ldvt * esz) % 16 || (a.ldo * esz) % 8) return "op_attention_view: ld alignment";
  if (a.flags & ~7) return "op_attention_view: unknown flags";
  if ((a.flags & 2) && !(a.flags & 1)) return "op_attention_view: flags bit 1 (MX) rides on bit 0 (fp8 P.V)";
  if ((a.flags & 1) && a.pos_bias) return "op_attention_view: pos_bias with an fp8 P.V flag";
  if ((a.flags & 1) && (a.bias || a.Skv % 64 != 0)) return "op_attention_view: the fp8 P.V path takes unmasked problems with Skv % 64 == 0";
  if ((a.flags & 2) && a.Skv % 128 != 0) return "op_attention_view: the MX fp8 P.V path takes Skv % 128 == 0";
  return nullptr;
}

}  // namespace tango

// Stand-alone run of attn_view_refusal() (tango_amd/csrc/attn_view_check.h), the host checker of tango_op_attention_view, for a sanitizer
// build without HIP or Python:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/attn_view_check_main.cpp -o attn_view_check && ./attn_view_check
// Walks every refusal once, then sweeps a grid of arguments (extreme ints included) and checks for each accepted set that the byte ranges
// attn_kernel can touch lie inside the buffers the hook allocates.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../tango_amd/csrc/attn_view_check.h"

using tango::AttnViewArgs;
using tango::attn_view_refusal;

static int failures = 0;

static void expect(const AttnViewArgs& a, const char* part, const char* what) {
  const char* r = attn_view_refusal(a);
  const bool ok = part ? (r && std::strstr(r, part)) : r == nullptr;
  if (!ok) {
    ++failures;
    std::printf("FAIL %s: got \"%s\", want %s%s\n", what, r ? r : "(accepted)", part ? "a message with " : "acceptance", part ? part : "");
  }
}

static AttnViewArgs good(int dtype) {
  AttnViewArgs a;
  a.dtype = dtype; a.B = 2; a.heads = 2; a.Sq = 128; a.Skv = 128; a.ldq = a.ldk = 256; a.k_col0 = 128; a.ldvt = 128; a.ldo = 128;
  a.pad_value = -7.0f; a.q_base = 0x1000; a.k_base = 0x1000 + 128 * (dtype ? 2 : 4); a.vt_base = 0x2000; a.o_base = 0x3000;
  return a;
}

// an accepted set keeps every access of the kernel inside [0, bytes) of its buffer
static void check_extents(const AttnViewArgs& a) {
  const int64_t esz = a.dtype ? 2 : 4, C = (int64_t)a.heads * 64;
  const bool one = a.k_col0 >= 0;
  const int64_t qbytes = (int64_t)a.B * a.Sq * a.ldq * esz, kbytes = one ? qbytes : (int64_t)a.B * a.Skv * a.ldk * esz;
  const int64_t vbytes = (int64_t)a.B * C * a.ldvt * esz, obytes = (int64_t)a.B * a.Sq * a.ldo * esz;
  const int64_t kcol = one ? a.k_col0 : 0;
  const int64_t q_end = (((int64_t)a.B * a.Sq - 1) * a.ldq + C) * esz;
  const int64_t k_end = (((int64_t)a.B * a.Skv - 1) * a.ldk + kcol + C) * esz;
  const int64_t v_cols = (a.ldvt * esz / 16) * (16 / esz);                     // the masked form reads whole 16-byte pieces below ldvt
  const int64_t v_end = (((int64_t)a.B * C - 1) * a.ldvt + v_cols) * esz;
  const int64_t o_end = (((int64_t)a.B * a.Sq - 1) * a.ldo + a.o_col0 + C) * esz;
  const int64_t off32 = 127 * (a.ldk > a.ldvt ? a.ldk : a.ldvt) * esz + 256;   // the largest per-thread offset: row < 128
  if (q_end > qbytes || k_end > kbytes || v_end > vbytes || o_end > obytes || off32 >= (1ll << 32) || kcol * esz % 16 || a.o_col0 * esz % 8) {
    ++failures;
    std::printf("FAIL extents: dtype %d B %d heads %d Sq %d Skv %d ldq %lld ldk %lld k_col0 %lld ldvt %lld ldo %lld o_col0 %lld\n", a.dtype, a.B,
                a.heads, a.Sq, a.Skv, (long long)a.ldq, (long long)a.ldk, (long long)a.k_col0, (long long)a.ldvt, (long long)a.ldo, (long long)a.o_col0);
  }
}

int main() {
  for (int dt = 0; dt < 3; ++dt) {
    const int64_t esz = dt ? 2 : 4;
    AttnViewArgs a = good(dt);
    expect(a, nullptr, "the good case");
    a = good(dt); a.pad_value = std::numeric_limits<float>::quiet_NaN(); expect(a, "finite", "NaN pad");
    a = good(dt); a.pad_value = std::numeric_limits<float>::infinity(); expect(a, "finite", "Inf pad");
    a = good(dt); a.pad_value = -std::numeric_limits<float>::infinity(); expect(a, "finite", "-Inf pad");
    a = good(dt); a.k_col0 = -1; a.ldq = 127; expect(a, "at least heads * 64", "ldq < C");
    a = good(dt); a.k_col0 = -1; a.ldk = 120; expect(a, "at least heads * 64", "ldk < C");
    a = good(dt); a.ldo = 64; expect(a, "at least heads * 64", "ldo < C");
    a = good(dt); a.k_col0 = 136; expect(a, "exceeds ldq", "k_col0 + C > ldq");
    a = good(dt); a.k_col0 = 64; expect(a, "inside the columns of q", "k over q");
    a = good(dt); a.k_col0 = -2; expect(a, "k_col0", "k_col0 < -1");
    a = good(dt); a.Sq = 64; expect(a, "Sq == Skv", "one buffer, Sq != Skv");
    a = good(dt); a.ldk = 264; expect(a, "ldk == ldq", "one buffer, ldk != ldq");
    a = good(dt); a.ldo = 136; a.o_col0 = 16; expect(a, "exceeds ldo", "o_col0 + C > ldo");
    a = good(dt); a.o_col0 = -8; expect(a, "negative", "o_col0 < 0");
    a = good(dt); a.ldvt = 120; expect(a, "round8", "ldvt < round8(Skv)");
    a = good(dt); a.Skv = a.Sq = 121; a.ldvt = 120; expect(a, "round8", "ldvt < round8(121)");
    a = good(dt); a.q_base += 8; expect(a, "16-byte", "q base");
    a = good(dt); a.k_base += 8; expect(a, "16-byte", "k base");
    a = good(dt); a.vt_base += 4; expect(a, "16-byte", "v^T base");
    a = good(dt); a.o_base += 4; expect(a, "8-byte", "o base");
    a = good(dt); a.o_base += 8; expect(a, nullptr, "o base 8-byte aligned");
    a = good(dt); a.k_col0 = -1; a.ldq = 128 + 8 / esz; expect(a, "ld alignment", "ldq");
    a = good(dt); a.ldvt = 128 + 8 / esz; expect(a, "ld alignment", "ldvt");
    a = good(dt); a.ldo = 128 + 4 / esz; expect(a, "ld alignment", "ldo");
    a = good(dt); a.ldo = 1 << 20; expect(a, "65536", "huge ldo");
    a = good(dt); a.B = 1 << 20; a.Sq = a.Skv = a.ldvt = 1 << 10; expect(a, "too large", "huge rows");
    a = good(dt); a.flags = 1; a.pos_bias = true; expect(a, "pos_bias with an fp8", "fp8 + pos_bias");
    a = good(dt); a.flags = 3; a.pos_bias = true; expect(a, "pos_bias with an fp8", "mx + pos_bias");
    a = good(dt); a.flags = 1; a.bias = true; expect(a, "unmasked", "fp8 + bias");
    a = good(dt); a.flags = 3; a.Sq = a.Skv = 192; a.ldvt = 192; expect(a, "128", "mx, Skv % 128");
    a = good(dt); a.flags = 2; expect(a, "rides on", "mx without fp8");
    a = good(dt); a.flags = 8; expect(a, "unknown flags", "flag 8");
    a = good(dt); a.dtype = 3; expect(a, "bad dtype", "dtype 3");
    a = good(dt); a.heads = 0; expect(a, "bad sizes", "heads 0");
  }
  // sweep: whatever is accepted stays inside its buffers; extreme values must not overflow the checker's own arithmetic (UBSan)
  const int big = std::numeric_limits<int>::max(), small = std::numeric_limits<int>::min();
  const int sizes[] = {small, -1, 0, 1, 7, 64, 130, 576, 65536, big};
  const int lds[] = {small, -8, 0, 63, 64, 66, 68, 72, 128, 132, 136, 256, 65536, 65544, big};
  const int cols[] = {small, -2, -1, 0, 2, 4, 8, 64, 128, big};
  long accepted = 0, asked = 0;
  for (int dt = 0; dt < 3; ++dt)
    for (int heads : {1, 2, big})
      for (int S : sizes)
        for (int Skv : {S, 7, 64})
          for (int ldq : lds)
            for (int ldk : {ldq, 64, 72, 128})
              for (int kc : cols)
                for (int ldo : lds)
                  for (int oc : cols) {
                    AttnViewArgs a;
                    a.dtype = dt; a.B = 2; a.heads = heads; a.Sq = S; a.Skv = Skv; a.ldq = ldq; a.ldk = ldk; a.k_col0 = kc;
                    a.ldvt = Skv > 0 ? ((int64_t)Skv + 7) / 8 * 8 + (dt ? 8 : 4) : 0; a.ldo = ldo; a.o_col0 = oc; a.pad_value = -7.0f;
                    a.q_base = 0x1000; a.k_base = 0x1000 + (kc > 0 ? (uintptr_t)kc * (dt ? 2 : 4) : 0); a.vt_base = 0x2000;
                    a.o_base = 0x3000 + (oc > 0 ? (uintptr_t)oc * (dt ? 2 : 4) : 0);
                    ++asked;
                    if (!attn_view_refusal(a)) { ++accepted; check_extents(a); }
                  }
  std::printf("attn_view_refusal: %ld argument sets, %ld accepted, %d failures\n", asked, accepted, failures);
  return failures ? 1 : 0;
}

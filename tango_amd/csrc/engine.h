// Internal engine classes (host side).  The public surface is include/tango_engine.h.
#pragma once
#include <array>
#include <functional>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/tango_engine.h"
#include "common.h"

namespace tango {

using Op = std::function<int(hipStream_t)>;

struct Program {
  std::vector<Op> ops;
  std::vector<std::string> labels;   // parallel to ops (per-op profiling)
  std::vector<double> flops;
  int run(hipStream_t s) const {
    for (const auto& o : ops) TANGO_TRY(o(s));
    return 0;
  }
  // eager run with HIP events around every op; appends "label<TAB>ms<TAB>gflop" lines to `report`
  int run_profiled(hipStream_t s, std::string& report) const;
};

// bump allocator over one hipMalloc'd slab; build is run twice (measure, then real)
struct Arena {
  char* base = nullptr;
  size_t off = 0, peak = 0;
  void* alloc(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    void* p = base ? (void*)(base + off) : (void*)(uintptr_t)(0x1000 + off);
    off += bytes;
    if (off > peak) peak = off;
    return p;
  }
  size_t mark() const { return off; }
  void release(size_t m) { off = m; }
};

struct TView {
  void* p = nullptr;
  int64_t ld = 0;
  int C = 0;
};

struct WMat {            // packed GEMM weight [N][Kp] (engine dtype) + fp32 bias
  void* W = nullptr;
  float* b = nullptr;
  int N = 0, K = 0, Cin = 0, taps = 1;
  int64_t Kp = 0;
  bool im2col = false;   // 3x3 conv with tiny Cin: K = 9*Cin zero-padded to Kp, A comes from im2col
  void* Wph = nullptr;   // UNet upsampler convs, 16-bit engines: [4 phases][N][4 Cin] summed 2x2-tap phase weights (launch_pack_ups_phase)
  // LayerNorm-folded copy (linear_stream.hip): W' = W*gamma, b' = b + W.beta, wsum[n] = sum_k W'[n][k]
  void* Wln = nullptr;
  float* bln = nullptr;
  float* wsum = nullptr;
};
struct WNorm {
  float* g = nullptr;
  float* b = nullptr;
  int C = 0;
  float eps = 1e-5f;
};
struct WLinF32 {         // fp32 [N][K] (time-embedding path stays fp32)
  float* W = nullptr;
  float* b = nullptr;
  int N = 0, K = 0;
};

struct ResW {
  int cin = 0, cout = 0;
  WNorm n1, n2;
  WMat c1, c2, sc;
  bool has_sc = false;
  bool has_temb = false;
  WLinF32 temb;
  float* temb_table = nullptr;  // [max_steps][cout] fp32, filled per denoise call
};
struct XfW {             // Transformer2DModel with one BasicTransformerBlock
  int C = 0, heads = 0;
  int cond = 0;          // which condition its cross-attention reads: 0 text, 1 beat, 2 chord (Music UNet: attentions / attentions2 / attentions3)
  WNorm gn, ln1, ln2, ln3;
  WMat proj_in, qkv, o1, q2, kv2, o2, ff1, ff2, proj_out;
  // fused cross-attention block (xattn.hip; C = 320 on 16-bit engines): LayerNorm-folded to_q with rows permuted per head
  void* q2p = nullptr;
  float* bq2p = nullptr;
  float* wsum2p = nullptr;
};
struct VaeAttnW {
  WNorm gn;
  WMat qk, v, proj;
};
struct ConvTW {          // ConvTranspose1d decomposed into `stride` phase matrices
  int cin = 0, cout = 0, k = 0, u = 0, pad = 0;
  std::vector<WMat> phase;
  float* b = nullptr;
};
struct VocResW {
  int ch = 0, k = 0;
  std::vector<int> dil;
  std::vector<WMat> c1, c2;
};

struct Slot {
  std::string name;
  std::vector<int64_t> shape;
  bool set = false;
  std::function<int(const float*, hipStream_t)> pack;
};

// every plan (a workspace slab + its launch program, keyed by the call's shape) carries its size and a last-use stamp: the plan
// caches of an engine share ONE byte budget, least recently used plans are freed first (Engine::make_room; round 4 -- callers of
// tango.py:51-64 with ragged last batches and mixed prompt lengths used to accumulate ~0.44 GB per prompt without bound)
struct PlanMeta {
  size_t bytes = 0;
  uint64_t stamp = 0;
};
// the kinds of plan an engine caches: the first entry of a PlanKey, followed by the shape ints of the call
enum PlanKind { PLAN_UNET, PLAN_VAE_DEC, PLAN_VAE_ENC, PLAN_VOC, PLAN_T5, PLAN_STFT };
using PlanKey = std::array<int, 8>;
struct Plan {
  const PlanKind kind;
  PlanMeta meta;
  char* slab = nullptr;
  explicit Plan(PlanKind k) : kind(k) {}     // get_plan() passes the kind of the key
  virtual ~Plan() = default;
};

// how a UNet plan runs its batch (the last entry of its PlanKey)
enum class UNetMode {
  Whole = 1,       // one program for the whole batch
  TwoChains = 2,   // two half-batch chains (the plan is a parent with two children)
  CfgShared = 3,   // one program with the CFG-shared prefix (build_unet)
};

// the captured graphs of one update kernel: one denoise step, and k_steps of them back to back (round 5)
struct StepGraphs {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipGraph_t graph_k = nullptr;
  hipGraphExec_t exec_k = nullptr;
  int k_steps = 0;
};

struct UNetPlan : Plan {
  using Plan::Plan;
  UNetMode mode = UNetMode::Whole;
  int B2 = 0, L = 0;
  int H = 0;                // latent height of the call (the plan's images are H >> level rows of cfg.latent_w >> level pixels)
  int Lc[3] = {0, 0, 0};    // condition lengths: [0] text (== L), [1] beat, [2] chord (Music UNet only)
  Program pre, step;
  void* xin = nullptr;      // T  [B2*HW][8]
  float* eps = nullptr;     // f32 [B2*HW][out_ch]
  void* enc = nullptr;      // T  [B2*L][cross]       (== encs[0])
  float* bias = nullptr;    // f32 [B2*L]             (== biases[0])
  void* encs[3] = {nullptr, nullptr, nullptr};
  float* biases[3] = {nullptr, nullptr, nullptr};
  // single-key prefix (round 4): the first n_short samples attend to exactly ONE text key (the unconditional rows of a CFG batch are
  // T5("") = one valid token), so their text cross-attention output is the constant to_out(v_key) + b, independent of the query
  int n_short = 0;
  int* key0 = nullptr;      // i32 [B2]: index of that key per sample (entries >= n_short unused)
  // [masked][multistep][guided]: the update kernel is chosen at launch (launch_sched_step: DDPM and DDIM share one, the multistep rule has
  // its own, and the masked (inpainting) variants fuse the blend of the next loop index into either), so a graph captured with one
  // cannot replay a loop that needs another; everything else is shared.  [guided]: the table / rescale variants, with the two
  // statistics launches in front of the update (a default call replays the [.][.][0] graphs: today's kernel sequence)
  StepGraphs graphs[2][2][2];
  // a windowed call (Engine::denoise_windowed) runs this plan's step program with sched_window_kernel as its update: graphs of its own,
  // so that a plain call and a windowed call of one shape share the plan and each replays the graph that holds its own update kernel.
  // [weighted]: the kernel that weights its views by the block's table (timed prompts).  A linear and a ring call of one shape replay the
  // same graphs: the kernel reads g.ring from the call's block as it reads everything else, and the grid is the plan's in both modes.
  StepGraphs wgraphs[2];
  // Two independent chains (round 5; Engine::denoise): a "dual" plan owns only the UNet input / output buffers of the whole batch; its
  // two children run the first and the second half of the samples (no op of the UNet crosses samples) as two branches of the captured
  // graph, so that one branch's dispatch gaps and kernel tails are filled by the other's kernels.  A child takes xin / eps from its
  // parent (ext_*), owns its slab and program, and is never in the plan cache on its own (the parent's eviction frees all three slabs).
  std::unique_ptr<UNetPlan> child[2];
  void* ext_xin = nullptr;
  float* ext_eps = nullptr;
  unsigned* sync = nullptr;    // barrier words its cooperative kernels use (one set per chain: two chains may run such a kernel at once)
};
struct T5LayerW {          // T5Block of the encoder: self-attention + gated-GELU feed-forward (no biases anywhere)
  WNorm ln1, ln2;
  WMat qkv, o, wi, wo;     // qkv = fused [q; k; v] rows; wi = [wi_1 | wi_0] in the GLU interleave (value | gate)
};
struct T5Plan : Plan {
  using Plan::Plan;
  int B = 0, L = 0;
  Program prog;
  int64_t* ids = nullptr;   // [B*L]
  float* bias = nullptr;    // [B*L] additive key mask
  int* bucket = nullptr;    // [L*L] relative-position buckets (host-computed)
  float* pos_bias = nullptr;  // [heads][L][L]
  float* out = nullptr;     // [B*L][d_model] fp32
};
struct VaePlan : Plan {    // decoder, encoder and vocoder: plan-owned in/out staging buffers
  using Plan::Plan;
  int B = 0;
  int H = 0;                // decoder / encoder: latent height of the call
  Program prog;
  void* in = nullptr;
  void* out = nullptr;
  size_t in_bytes = 0, out_bytes = 0;
  int n_out = 0;            // vocoder: samples per item
};

struct StftPlan : Plan {   // wave -> log-mel front-end buffers for one (batch, n_samples)
  using Plan::Plan;
  int B = 0, N = 0, T = 0, Np = 0, Kp2 = 0, ldz = 0;
  float *in = nullptr, *xpad = nullptr, *Z = nullptr, *mag = nullptr, *mel_lin = nullptr, *mel = nullptr, *logmag = nullptr, *energy = nullptr;
};

class Engine {
 public:
  explicit Engine(const tango_config_t& c);
  ~Engine();
  int init();

  int set_weight(const char* name, const float* dev, const int64_t* shape, int ndim);
  int finalize_weights();
  int denoise(const tango_denoise_args_t& a, const tango_guidance_args_t* g, hipStream_t s);   // g may be null: scalar guidance, no rescale
  // long clips: a.latent_h is the canvas height, the UNet runs (cfg ? 2 : 1) * a.batch * V windows of height w.window_h per step.
  // ring (loops): the canvas rows are a ring (V = a.latent_h / w.stride views that wrap).  weighted (timed prompts): view_weights is a
  // HOST [w.window_h] table, a positive weight per local window row, and the update is the weighted mean; otherwise it is not read.
  int denoise_windowed(const tango_denoise_args_t& a, const tango_window_args_t& w, bool ring, const float* view_weights, bool weighted, hipStream_t s);
  // the tiled decode of such a canvas, cross-faded over the overlaps (round a ring's wrap point too); the vocoder on a ring of mel frames
  int vae_decode_windowed(const float* lat, float* mel, int B, int canvas_h, int window_h, int stride, bool ring, hipStream_t s);
  int vocode_ring(const float* mel, int16_t* wav, int B, int frames, int* n_samples, hipStream_t s);
  int vocoder_ring_context() const;     // mel frames of context vocode_ring pads each side with: the vocoder's receptive field
  struct Cond { const float* emb = nullptr; const uint8_t* mask = nullptr; int len = 0; const uint8_t* mask_host = nullptr; };
  // latent_h: the latent height of the call, 0 = cfg.latent_h (the width is always cfg.latent_w)
  int unet_forward(const float* sample, int64_t t, const Cond (&c)[3], float* out, int B2, int latent_h, hipStream_t s);
  int vae_decode(const float* lat, float* mel, int B, int latent_h, hipStream_t s);
  int vae_encode(const float* mel, float* moments, int B, int latent_h, hipStream_t s);
  int vocode(const float* mel, int16_t* wav, int B, int frames, int* n_samples, hipStream_t s);
  int vocoder_samples(int frames) const;
  int encode_text(const int64_t* ids, const uint8_t* mask, float* out, int B, int L, hipStream_t s);
  int mel_spectrogram(const float* wav, float* mel, float* logmag, float* energy, int B, int N, int* n_frames, hipStream_t s);
  int last_denoise_ms(float* total_ms, float* per_step_ms);
  int profile_unet(int B2, int L, int latent_h, std::string& report, hipStream_t s);
  int profile_vae(int B, int latent_h, std::string& report, hipStream_t s);                 // per-op timing of the mel-VAE decoder plan (round 6)
  int profile_vocoder(int B, int frames, std::string& report, hipStream_t s);  // ... of the HiFi-GAN plan
  // plan-cache budget (bytes of workspace slabs kept alive; default 64 GiB or TANGO_PLAN_BUDGET_MB) and its current use
  void set_plan_budget(size_t bytes) { plan_budget = bytes; }
  void drop_plans() { const size_t b = plan_budget; plan_budget = 0; (void)make_room(1); plan_budget = b; }   // frees every cached plan
  size_t plan_bytes_in_use() const { return plan_bytes; }
  int plan_count() const { return (int)plans.size(); }
  size_t ring_capacity() const { return ring_elems; }     // floats the multistep history holds (diagnostic)

  tango_config_t cfg;
  int dt = DT_F32;
  size_t esz = 4;
  std::vector<Slot> slots;
  std::unordered_map<std::string, int> slot_index;
  bool finalized = false;
  float last_total_ms = 0.f, last_step_ms = 0.f;
  double last_step_gflop = 0.0;  // executed GFLOP of one launch of the last denoise call's step program
  uint64_t coop_fallbacks = 0;   // workgroups of gn_coop_kernel that took the no-rendezvous fallback (diagnostic; results are unaffected)

 private:
  friend struct Builder;
  // ---- memory ----
  std::vector<void*> owned;
  void* dmalloc(size_t bytes);
  // ---- weight registration ----
  void reg_slot(const std::string& name, std::vector<int64_t> shape, std::function<int(const float*, hipStream_t)> pack);
  void reg_vec(const std::string& name, int n, float** dst);
  void reg_norm(const std::string& p, int C, float eps, WNorm& w);
  void reg_mat(const std::string& wname, int N, int K, WMat& w, bool alloc, int row_off, std::vector<int64_t> shape, bool geglu = false);
  void reg_linear(const std::string& p, int N, int K, WMat& w, bool bias);
  void reg_conv3x3(const std::string& p, int Cout, int Cin, WMat& w, bool ups_phase = false);
  void reg_conv1x1(const std::string& p, int Cout, int Cin, WMat& w);
  void reg_conv1d(const std::string& p, int Cout, int Cin, int k, WMat& w);
  void reg_convt1d(const std::string& p, int Cin, int Cout, int k, int u, ConvTW& w);
  void reg_linear_f32(const std::string& p, int N, int K, WLinF32& w);
  void reg_res(const std::string& p, int cin, int cout, int temb, float eps, ResW& w, bool vae);
  void reg_xf(const std::string& p, int C, int heads, int cross, XfW& w);
  int fold_ln(WMat& w, const WNorm& ln);
  void build_unet_weights();
  void build_vae_weights();
  void build_vae_enc_weights();
  void reg_vae_attn(const std::string& p, int C, VaeAttnW& w);
  void build_voc_weights();
  void build_t5_weights();
  void build_stft_weights();       // frontend.hip

  // ---- model weights ----
  // UNet
  WMat conv_in, conv_out;
  WNorm norm_out;
  WLinF32 time1, time2;
  // xf[j] is the site's text transformer; xf2 / xf3 are `attentions2` / `attentions3` of the Music blocks (empty otherwise)
  struct DownBlock { std::vector<ResW> res; std::vector<XfW> xf, xf2, xf3; bool has_ds = false; WMat ds; };
  struct UpBlock { std::vector<ResW> res; std::vector<XfW> xf, xf2, xf3; bool has_us = false; WMat us; };
  std::vector<DownBlock> down;
  std::vector<UpBlock> up;
  ResW mid_res0, mid_res1;
  XfW mid_xf, mid_xf2, mid_xf3;
  std::vector<ResW*> all_res;   // every UNet resblock (temb tables)
  std::vector<XfW*> all_xf;
  // VAE
  float* pqc_w = nullptr; float* pqc_b = nullptr;
  WMat vae_conv_in, vae_conv_out;
  ResW vae_mid1, vae_mid2;
  VaeAttnW vae_attn;
  struct VaeUp { std::vector<ResW> res; bool has_up = false; WMat up; };
  std::vector<VaeUp> vae_up;    // indexed by level
  WNorm vae_norm_out;
  // encoder (modules.py:419-543) + quant_conv
  struct VaeDown { std::vector<ResW> res; bool has_down = false; WMat down; };
  std::vector<VaeDown> vae_down;
  WMat vae_enc_conv_in, vae_enc_conv_out;
  ResW vae_enc_mid1, vae_enc_mid2;
  VaeAttnW vae_enc_attn;
  WNorm vae_enc_norm_out;
  float* qc_w = nullptr; float* qc_b = nullptr;
  // vocoder
  WMat voc_pre, voc_post;
  std::vector<ConvTW> voc_ups;
  std::vector<VocResW> voc_res;

  // wave -> log-mel front-end (frontend.hip)
  WMat stft_basis, stft_mel;
  int get_stft_plan(int B, int N, StftPlan** out);

  // text encoder
  float* t5_embed = nullptr;        // [vocab][d_model] fp32
  float* t5_rel_table = nullptr;    // [rel_buckets][heads] fp32
  std::vector<T5LayerW> t5_layers;
  WNorm t5_final_ln;
  int get_t5_plan(int B, int L, T5Plan** out);
  int build_t5(T5Plan& P, Arena& A, bool record);

  // ---- runtime state ----
  int* d_step = nullptr;
  unsigned* d_sync = nullptr;   // barrier words of the cooperative kernels (common.h: coop_sync_words()), zeroed once at init
  SchedParams* d_sched = nullptr;   // device copy of the current call's scheduler parameter block
  SchedWindowParams* d_wsched = nullptr;   // ... of the current windowed call's block (captured windowed steps read this one)
  float* d_wweights = nullptr;   // [kMaxLatentH] the current weighted call's view weights (the block's `weights` points here)
  int64_t* d_ts = nullptr;       // [max_steps]
  float* d_coef = nullptr;       // [max_steps][16] (DDPM / DDIM rows use the first 8 floats of a packed [N][8] table)
  float* d_bcoef = nullptr;      // [max_steps][2] add_noise scalars of the masked loop's blend (tango_denoise_args_t.blend_coef)
  float* d_ring = nullptr;       // multistep history [3][B][C][HW] fp32 of the call (hipMalloc'd, grown on demand; not in `owned`)
  size_t ring_elems = 0;         // its capacity in floats
  // guided calls (tango_guidance_args_t): one allocation, grown like d_ring, that holds the call's guidance table [N][B] fp32, the
  // statistics partials [B][chunks][4] fp64 and the rescale factors [B] fp32 (SchedParams gtable / gpart / gscale point into it)
  char* d_guide = nullptr;
  size_t guide_bytes = 0;
  float* d_sin = nullptr;        // [max_steps][ch0]
  float* d_t1 = nullptr;         // [max_steps][temb]
  float* d_temb = nullptr;       // [max_steps][temb]  silu(emb)
  std::vector<int64_t> temb_ts;  // cache key
  int max_steps = 1000;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipStream_t cap_stream = nullptr;
  // second chain of a dual plan: its capture stream, its eager stream, fork / join events (capture and eager pairs), barrier words
  hipStream_t cap_stream2 = nullptr, aux_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_fork_e = nullptr, ev_join_e = nullptr;
  unsigned* d_sync2 = nullptr;
  int last_steps = 0;

  // ---- host -> device staging without a host sync (round 4) ----
  // Small per-call tables (timesteps, scheduler coefficients, the SchedParams block, single-key indices) come from pageable /
  // transient host memory.  They are copied into engine-owned PINNED slots and uploaded with hipMemcpyAsync; a slot is reused
  // only after the event recorded behind its upload has fired, so neither the caller's buffer nor the slot can be overwritten
  // under a pending copy and `denoise` returns without waiting for the stream.
  struct HostSlot { void* buf = nullptr; hipEvent_t ev = nullptr; bool pending = false; };
  static constexpr int kHostSlots = 8;
  static constexpr size_t kHostSlotBytes = 64 << 10;
  HostSlot hslots[kHostSlots];
  int hslot_next = 0;
  int stage_h2d(void* dst_dev, const void* src_host, size_t bytes, hipStream_t s);

  // ---- the plan cache: every kind of plan in one map, one LRU byte budget ----
  // keys: UNet (B2, L_text, L_beat, L_chord, n_short, mode, H); VAE decoder / encoder (B, H); vocoder (B, frames); T5 (B, L); STFT (B, N)
  std::map<PlanKey, std::unique_ptr<Plan>> plans;
  size_t plan_budget = (size_t)64 << 30, plan_bytes = 0;
  uint64_t plan_clock = 0;
  void touch(PlanMeta& m) { m.stamp = ++plan_clock; }
  int make_room(size_t need);             // frees least-recently-used plans until plan_bytes + need <= plan_budget (or nothing is left)
  bool evict_lru();
  int alloc_slab(char** slab, size_t bytes, PlanMeta& m, bool zero);   // on out-of-memory: evicts LRU plans and retries
  void free_plan(Plan& P);                // graphs and children of a UNet plan, the slab; gives the bytes back to the budget
  // `build` lays the plan out in an arena and, when `record`, records its program.  It runs twice: against a null arena to measure,
  // then on the slab allocated from that measure (+ 256 bytes of slack; zero-filled when `zero`).  A plan that fails is freed here.
  int build_plan(Plan& P, bool zero, const std::function<int(Arena&, bool record)>& build);
  // the cached plan of `key`, or a new one: `init` fills in the shape fields, `build` goes through build_plan(), `post` (optional)
  // runs on the built plan.  The plan enters the cache only when all of that succeeded (it is freed otherwise), so a plan under
  // construction is invisible to the evictions its own allocation may trigger.
  template <class P>
  int get_plan(const PlanKey& key, bool zero, P** out, const std::function<void(P&)>& init,
               const std::function<int(P&, Arena&, bool record)>& build, const std::function<int(P&)>& post = nullptr) {
    auto it = plans.find(key);
    if (it != plans.end()) { touch(it->second->meta); *out = static_cast<P*>(it->second.get()); return 0; }
    if (!finalized) TANGO_FAIL("engine: weights not finalized");
    std::unique_ptr<P> p(new P((PlanKind)key[0]));
    init(*p);
    TANGO_TRY(build_plan(*p, zero, [&](Arena& A, bool record) { return build(*p, A, record); }));
    if (post)
      if (int rc = post(*p)) { free_plan(*p); return rc; }
    *out = p.get();
    plans[key] = std::move(p);
    return 0;
  }

  int ensure_temb(const int64_t* ts_host, int n, hipStream_t s);
  static constexpr int kMaxLatentH = 4096;
  int resolve_h(int latent_h, bool unet, int* H) const;
  int get_unet_plan(int B2, int L, int Lbeat, int Lchord, int n_short, int H, UNetPlan** out, UNetMode mode = UNetMode::Whole);
  int build_unet_plan(UNetPlan& P, Arena& A, bool record);   // build_unet, or the parent and the two children of a two-chain plan
  bool cfg_shared_ok(int B2, int n_short) const;
  // how a guidance / plain batch of B2 UNet rows runs; profile_unet() asks with two_chains_ok = false
  UNetMode unet_mode_for(int B2, int n_short, bool cfg_on, bool two_chains_ok) const;
  // which update closes a step: the kernel is fixed when a step is captured
  // weighted: a windowed step that weights its views by the block's table (linear or ring is the block's to say, not the kernel's)
  struct StepKind { int rule = 0; bool masked = false, guided = false, windowed = false, weighted = false; };
  int run_step(const UNetPlan& P, const StepKind& k, hipStream_t st, hipStream_t st2, hipEvent_t fork, hipEvent_t join);
  int capture_steps(const UNetPlan& P, const StepKind& k, int n, hipGraph_t* g_out, hipGraphExec_t* x_out);
  // the loop of a denoise call once its blocks, conditions and first UNet input are in place: captures what G lacks, replays or runs eagerly
  int run_loop(UNetPlan& P, StepGraphs& G, const StepKind& k, int num_steps, bool use_graph, hipStream_t s);
  int single_key_prefix(const uint8_t* mask_dev, const uint8_t* mask_host, int B2, int L, std::vector<int>& key0, hipStream_t s);
  int build_unet(UNetPlan& P, Arena& A, bool record);
  int get_vae_plan(int B, int H, VaePlan** out);
  int build_vae(VaePlan& P, Arena& A, bool record);
  int get_vae_enc_plan(int B, int H, VaePlan** out);
  int build_vae_enc(VaePlan& P, Arena& A, bool record);
  int get_voc_plan(int B, int frames, VaePlan** out);
  int build_voc(VaePlan& P, Arena& A, bool record, int frames);
  int bind_text(UNetPlan& P, const Cond (&c)[3], const std::vector<int>& key0, hipStream_t s);
  int bind_conditions(UNetPlan& P, const Cond (&c)[3], const std::vector<int>& key0, hipStream_t s);   // bind_text per chain
};

}  // namespace tango

// the opaque handle of include/tango_engine.h
struct tango_engine { tango::Engine* e; };

/* tango_engine.h -- C ABI of the MI355X-native Tango text-to-audio inference engine.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference has no C plugin API:
 * its callers are Python duck-typed call sites.  Every entry point below names the
 * reference interface it replaces (paths relative to the reference tree):
 *
 *   tango_engine_denoise        AudioDiffusion.inference loop body        models.py:224-249
 *                               + DDPMScheduler.step                       mustango/diffusers/src/diffusers/schedulers/scheduling_ddpm.py:254-349
 *                               (+ DDIMScheduler.step                      .../scheduling_ddim.py:238-360)
 *                               (+ DPMSolverMultistepScheduler.step        .../scheduling_dpmsolver_multistep.py:429-495)
 *   tango_engine_denoise_windows  StableDiffusionPanoramaPipeline's loop    mustango/diffusers/src/diffusers/pipelines/stable_diffusion/pipeline_stable_diffusion_panorama.py:614-652
 *   tango_engine_vae_decode_tiled_h  AutoencoderKL.tiled_decode             mustango/diffusers/src/diffusers/models/autoencoder_kl.py:255-296
 *   tango_engine_unet_forward   UNet2DConditionModel.forward             mustango/diffusers/src/diffusers/models/unet_2d_condition.py:520-707
 *   tango_engine_unet_forward_music  UNet2DConditionModelMusic.forward      mustango/diffusers/src/diffusers/models/unet_2d_condition_music.py:536-757
 *   tango_engine_vae_decode     AutoencoderKL.decode_first_stage           audioldm/variational_autoencoder/autoencoder.py:116-124,60-64
 *   tango_engine_vae_encode     AutoencoderKL.encode (encode_first_stage)  audioldm/variational_autoencoder/autoencoder.py:52-58,112-113
 *   tango_engine_vocode         AutoencoderKL.decode_to_waveform           audioldm/variational_autoencoder/autoencoder.py:66-69
 *                               -> vocoder_infer                           audioldm/hifigan/utilities.py:76-86
 *   tango_engine_mel_spectrogram  TacotronSTFT.mel_spectrogram            audioldm/audio/stft.py:164-186 (+ STFT.transform :52-85)
 *   tango_engine_encode_text    T5EncoderModel forward (text_encoder(...)[0])  models.py:139-141,279-281,291-293
 *   tango_engine_set_weight     load_state_dict of pytorch_model_main.bin / pytorch_model_vae.bin   tango.py:22-28
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  Tensor arguments are CALLER-OWNED DEVICE
 *     pointers (contiguous, the reference's own shapes/layouts: NCHW fp32 latents, [B,L,d] fp32
 *     embeddings, bool masks as uint8).  The engine never frees caller memory.
 *   - `stream` is a hipStream_t passed as void* (the caller's current stream); all work is enqueued
 *     on it and is asynchronous unless stated.
 *   - every function returns 0 on success, non-zero on failure; tango_last_error() returns the
 *     message for the calling thread.  The Python shim re-raises ValueError / RuntimeError with the
 *     reference's conditions (e.g. num_inference_steps > num_train_timesteps).
 *   - a handle is not re-entrant; data-parallel use = one handle per GPU / process.
 */
#ifndef TANGO_ENGINE_H
#define TANGO_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TANGO_DTYPE_F32 0
#define TANGO_DTYPE_F16 1
#define TANGO_DTYPE_BF16 2

#define TANGO_PRED_EPSILON 0
#define TANGO_PRED_SAMPLE 1
#define TANGO_PRED_V 2

#define TANGO_RULE_DDPM 0
#define TANGO_RULE_DDIM 1
/* multistep DPM-Solver / DPM-Solver++ (mustango/diffusers/src/diffusers/schedulers/scheduling_dpmsolver_multistep.py:124-495):
 * deterministic (no step noise, `noise` must be NULL, `clip_sample` 0), coefficient rows 16 floats wide (coef_width = 16):
 *   [0] alpha_s0  [1] sigma_s0      conversion of the guided output (x0 for DPM-Solver++, eps for DPM-Solver)
 *   [2] kx  [3] c0  [4] c1  [5] c2  signed update coefficients (the fork's subtracted terms stored negated)
 *   [6] 1/r0  [7] 1/r1  [8] r0/(r0+r1)  [9] 1/(r0+r1)
 *   [10] effective order of the step (1, 2 or 3)  [11] algorithm: 0 DPM-Solver++, 1 DPM-Solver (the same in every row)
 *   [12..15] 0
 * update: order 1  x' = kx*x + c0*D0
 *         order 2  x' = (kx*x + c0*D0) + c1*D1                     D1 = (1/r0)*(m0 - m1)
 *         order 3  x' = ((kx*x + c0*D0) + c1*D1) + c2*D2           D1_0 = (1/r0)*(m0 - m1), D1_1 = (1/r1)*(m1 - m2),
 *                  D1 = D1_0 + (r0/(r0+r1))*(D1_0 - D1_1),  D2 = (1/(r0+r1))*(D1_0 - D1_1)
 * with D0 = m0 the converted output of this step and m1, m2 those of the two steps before (tango_amd/scheduler.py
 * DPMSolverMultistepScheduler.coef_table builds the table). */
#define TANGO_RULE_DPM_MULTISTEP 2

#define TANGO_MAX_LEVELS 8

typedef struct tango_engine tango_engine_t;

/* Mirrors configs/diffusion_model_config.json + mustango/configs/vae_config.json (ddconfig) +
 * HIFIGAN_16K_64 (audioldm/hifigan/utilities.py:9-39).  A component with n_levels == 0 / n_ups == 0
 * is not built. */
typedef struct tango_config {
  int32_t dtype;                              /* TANGO_DTYPE_*: storage/MFMA operand type; accumulation & statistics are fp32 */
  /* UNet2DConditionModel */
  int32_t unet_levels;                        /* len(block_out_channels) */
  int32_t unet_channels[TANGO_MAX_LEVELS];    /* block_out_channels */
  int32_t unet_heads[TANGO_MAX_LEVELS];       /* "attention_head_dim" (= head COUNT; head_dim is 64) */
  int32_t unet_cross_attn[TANGO_MAX_LEVELS];  /* 1 if down block i is CrossAttnDownBlock2D */
  int32_t unet_layers_per_block;
  int32_t unet_in_channels, unet_out_channels;
  int32_t unet_cross_dim;                     /* cross_attention_dim (1024 FLAN-T5-large, 2048 XL) */
  int32_t unet_groups;                        /* norm_num_groups */
  float unet_eps;                             /* norm_eps */
  int32_t unet_flip_sin_to_cos;
  float unet_freq_shift;
  int32_t latent_h, latent_w;                 /* 256, 16 (models.py:259-260) */
  /* mel-VAE decoder */
  int32_t vae_levels;                         /* len(ch_mult) */
  int32_t vae_ch;
  int32_t vae_ch_mult[TANGO_MAX_LEVELS];
  int32_t vae_num_res_blocks;
  int32_t vae_z_channels, vae_embed_dim, vae_out_ch;
  float vae_scale_factor;
  /* HiFi-GAN */
  int32_t voc_n_ups;
  int32_t voc_rates[TANGO_MAX_LEVELS];
  int32_t voc_kernels[TANGO_MAX_LEVELS];
  int32_t voc_initial_channel;
  int32_t voc_num_mels;
  int32_t voc_n_resblocks;                    /* len(resblock_kernel_sizes) == 3 */
  int32_t voc_res_kernels[4];
  int32_t voc_res_dilations[4][4];            /* [kernel idx][pair idx]; 0-terminated rows */
  /* FLAN-T5 encoder (transformers T5EncoderModel; reference call sites models.py:98-100,129-147,266-305).  Built when
   * t5_layers > 0; weights are the `text_encoder.*` tensors of pytorch_model_main.bin (HF key names). */
  int32_t t5_layers;                          /* num_layers (24 for flan-t5-large / -xl) */
  int32_t t5_d_model, t5_d_kv, t5_heads, t5_d_ff, t5_vocab;   /* d_kv must be 64 */
  int32_t t5_rel_buckets, t5_rel_max_distance;                /* relative_attention_num_buckets (32), _max_distance (128) */
  float t5_eps;                               /* layer_norm_epsilon (1e-6) */
  /* mel-VAE encoder (modules.py:419-543 + quant_conv, autoencoder.py:38,52-58): built when vae_encoder != 0 (needs the
   * vae_* fields above); weights are the `encoder.*` / `quant_conv.*` tensors of pytorch_model_vae.bin */
  int32_t vae_encoder;
  int32_t vae_in_channels;                    /* ddconfig["in_channels"] (1) */
  /* wave -> log-mel front-end (audioldm/audio/stft.py:136-186 TacotronSTFT; config keys of stft_config.json / models.py:40-47):
   * built when stft_filter_length > 0 (fp32 engines only); weights are the module's buffers `mel_basis` [n_mel, n_fft/2+1] and
   * `stft_fn.forward_basis` [2*(n_fft/2+1), 1, n_fft] (pytorch_model_stft.bin, tango.py:23-27) */
  int32_t stft_filter_length, stft_hop_length, stft_n_mel;
  /* Mustango's UNet2DConditionModelMusic (mustango/diffusers/src/diffusers/models/unet_2d_condition_music.py; config
   * mustango/configs/music_diffusion_model_config.json: CrossAttn{Down,Up}Block2DMusic / UNetMidBlock2DCrossAttnMusic): every
   * cross-attention site holds THREE Transformer2DModels applied in sequence -- `attentions` (text), `attentions2` (beat
   * embeddings), `attentions3` (chord embeddings), unet_2d_blocks.py:1199-1260,715-757,2372-2436.  All three conditions have
   * width unet_cross_dim. */
  int32_t unet_music;
  /* BASELINE config 5 ("bf16 + fp8 MFMA attention"): != 0 runs the P.V product of the UNet's self-attention sites on
   * v_mfma_f32_16x16x32_fp8_fp8 (P and V as OCP e4m3, fp32 accumulation, fp32 softmax statistics; Q.K^T stays in `dtype`).
   * 16-bit engines only.  Measured deviation: DESIGN.md section 3.  2 = the same product on the MX instruction
   * v_mfma_scale_f32_16x16x128_f8f6f4 (128 keys per MFMA, unit block scales, twice the matrix-pipe rate) at the sites whose sequence
   * length is a multiple of 128; same roundings. */
  int32_t unet_attn_fp8;
} tango_config_t;

typedef struct tango_denoise_args {
  float* latents;              /* in/out  [B, C_lat, H, W] fp32 NCHW: initial noise * init_noise_sigma in, x_0 out */
  const float* prompt_embeds;  /* [B2, L, d] fp32, B2 = 2B ([uncond; cond], models.py:301) when cfg, else B */
  const uint8_t* prompt_mask;  /* [B2, L] bool (1 = attend), may be NULL (no mask) */
  int32_t batch;               /* B */
  int32_t text_len;            /* L */
  int32_t num_steps;           /* N */
  const int64_t* timesteps;    /* HOST [N] (DDPMScheduler.set_timesteps, scheduling_ddpm.py:184-204) */
  const float* coef;           /* HOST [N][coef_width]; DDPM / DDIM: [N][8] sqrt(abar_t), sqrt(1-abar_t), coef_x0, coef_xt, sigma,
                                * sqrt(abar_prev), dir_coef, 0; TANGO_RULE_DPM_MULTISTEP: [N][16] (layout above) */
  float guidance_scale;        /* CFG is on when > 1.0 (models.py:213) */
  int32_t prediction_type;     /* TANGO_PRED_* */
  int32_t rule;                /* TANGO_RULE_* */
  int32_t clip_sample;
  float clip_sample_range;
  const float* noise;          /* device [N][B, C_lat, H, W] fp32 injected step noise (parity mode) or NULL -> device Philox */
  uint64_t seed;               /* Philox key when noise == NULL */
  int32_t sample_offset;       /* global index of local sample 0 (keeps Philox noise independent of the DP sharding) */
  int32_t use_graph;           /* 1: replay the captured hipGraph of the UNet step; 0: eager launches */
  /* Music UNet only (cfg.unet_music; mustango/models.py:540-598 MusicAudioDiffusion.inference): beat / chord condition
   * embeddings [B2, beat_len | chord_len, d] fp32 with bool masks [B2, len] (may be NULL), ordered [uncond; cond] like
   * prompt_embeds (mustango/models.py:650-740).  Ignored (may be NULL / 0) for the plain UNet. */
  const float* beat_embeds;
  const uint8_t* beat_mask;
  int32_t beat_len;
  const float* chord_embeds;
  const uint8_t* chord_mask;
  int32_t chord_len;
  /* optional HOST copy of prompt_mask (bool [rows, text_len], the tokenizer's attention mask before it was uploaded).  The engine
   * picks its plan from the mask's structure (the unconditional rows of a CFG batch keep one key, models.py:282-289); with the host
   * copy it does so without reading the device mask back, i.e. without a host sync on `stream`.  NULL: read-back (one sync). */
  const uint8_t* prompt_mask_host;
  /* floats per row of `coef`: 0 means 8 (DDPM / DDIM); 16 for TANGO_RULE_DPM_MULTISTEP */
  int32_t coef_width;
  /* masked-latent inpainting (audioldm/ldm.py:724-818 generate_sample_masked, audioldm/latent_diffusion/ddim.py:210-217), any rule:
   * before the UNet call of every loop index i (i = 0 included, on the initial latents; none after the last step)
   *   x = (sqrt(abar_i) * x0 + sqrt(1 - abar_i) * n_i) * m + (1 - m) * x
   * i.e. the fork's add_noise (scheduling_ddpm.py:351-371) of the known latents x0 at t_i, kept where m = 1.
   * known_latents: device [B, C_lat, H, W] fp32 (scale_factor * posterior sample); NULL = no masking (the fields below unused).
   * latent_mask:   device [B, 1, H, W] fp32 (broadcast over channels; 1 keeps the known audio, 0 regenerates it).
   * blend_coef:    HOST [N][2] = sqrt(abar_t_i), sqrt(1 - abar_t_i) (tango_amd/scheduler.py blend_table()).
   * blend_noise:   device [N][B, C_lat, H, W] fp32 n_i, or NULL -> device Philox on the step noise's key and counter layout with bit
   *                31 of the step word set (tango_op_philox_normal_blend), a stream disjoint from the step noise.  Allowed with every
   *                rule: it is not step noise. */
  const float* known_latents;
  const float* latent_mask;
  const float* blend_coef;
  const float* blend_noise;
  /* latent height H of this call: latents, noise, known_latents, latent_mask and blend_noise are [.., H, latent_w].  0 = the
   * configured tango_config_t.latent_h.  A multiple of 8 << (unet_levels - 1) (an error otherwise); the plan cache keys on it. */
  int32_t latent_h;
} tango_denoise_args_t;

const char* tango_last_error(void);
const char* tango_version(void);

int tango_engine_create(const tango_config_t* cfg, tango_engine_t** out);
void tango_engine_destroy(tango_engine_t* h);

/* number of parameter tensors the engine expects / name of the i-th one (reference state_dict keys,
 * "unet." prefix for the UNet as in pytorch_model_main.bin, plain keys for pytorch_model_vae.bin). */
int tango_engine_num_weights(tango_engine_t* h);
const char* tango_engine_weight_name(tango_engine_t* h, int i);
/* fp32 DEVICE tensor in the reference layout (Conv OIHW, Linear [out,in], ConvTranspose1d [in,out,k]);
 * the engine packs its own copy. `shape`/`ndim` are validated. */
int tango_engine_set_weight(tango_engine_t* h, const char* name, const float* dev_ptr, const int64_t* shape, int ndim);
/* fails (listing the first missing key) unless every expected tensor has been set */
int tango_engine_finalize_weights(tango_engine_t* h);

int tango_engine_denoise(tango_engine_t* h, const tango_denoise_args_t* args, void* stream);

/* Guidance beyond one scalar (tango_denoise_args_t itself is frozen: its last field stays latent_h).
 * table:   HOST [N][B] fp32 or NULL.  Entry [i][b] is the guidance scale of latents row b at loop index i; it replaces
 *          args->guidance_scale, which is then not read.  A table always runs the [uncond; cond] batch (prompt_embeds hold 2B rows,
 *          whatever the entries): 1.0 gives the conditional output, 0.0 the unconditional one.  Entries must be finite and >= 0.
 * rescale: phi in [0, 1], the guidance rescale of Lin et al. 2023 (section 3.4; diffusers' guidance_rescale).  Per sample b and step,
 *          over the n = C_lat * H * W values of the model output (u, c the unconditional and the conditional half, g the scale):
 *            cfg = u + g * (c - u)                  as without it (models.py:246)
 *            s_b = std(c) / std(cfg)                unbiased (n - 1), like torch.std
 *            v   = phi * (cfg * s_b) + (1 - phi) * cfg
 *          and the scheduler rule runs on v.  Each line is evaluated in fp32 in that order without FMA contraction (1 - phi is an fp32
 *          subtraction); s_b comes from fp64 sums about the sample's first element, added in a fixed order, so it does not depend on
 *          the batch size, the row of the sample or sample_offset.  std(cfg) == 0 gives s_b = 1 where the formula gives NaN: the one
 *          deviation.  phi > 0 needs guidance: a table, or guidance_scale > 1.
 * With guide NULL, or table NULL and rescale 0, the call is tango_engine_denoise: the same kernels and the same bits.  Otherwise every
 * step runs two small statistics launches and a table-reading variant of the update kernel, in a captured graph of its own; phi and
 * the table are read from device memory refreshed per call, so one captured graph serves every phi and every table. */
typedef struct tango_guidance_args {
  const float* table;          /* HOST [N][B] or NULL */
  float rescale;
} tango_guidance_args_t;
int tango_engine_denoise_guided(tango_engine_t* h, const tango_denoise_args_t* args, const tango_guidance_args_t* guide, void* stream);
/* host-side query, no GPU needed: "" when tango_engine_denoise_guided accepts these arguments as far as its argument checks go (no
 * engine state: shapes against the configuration are checked by the call itself), else the message it fails with: rescale outside
 * [0, 1] or NaN, rescale > 0 without guidance, a table entry negative or not finite, and every refusal of tango_engine_denoise's own
 * checks (rule, coef_width, multistep table rows, masking pointers).  Reads args->coef (multistep rule) and guide->table. */
const char* tango_debug_denoise_guided_check(const tango_denoise_args_t* args, const tango_guidance_args_t* guide);

/* Clips longer than the UNet's trained length: MultiDiffusion (Bar-Tal et al. 2023) windows in time, the fork's panorama pipeline
 * (mustango/diffusers/src/diffusers/pipelines/stable_diffusion/pipeline_stable_diffusion_panorama.py:442-456 get_views, :614-652 the per-step
 * loop) fused into the engine's step (tango_denoise_args_t itself is frozen).
 * Geometry: the canvas is args->latents [B, C_lat, H, latent_w] with H = args->latent_h (> 0; noise is [N][B, C_lat, H, latent_w]); window_h = Hw
 * is a UNet height, 1 <= stride = s <= Hw, and (H - Hw) % s == 0 -- the views cover the canvas exactly (get_views floors and leaves a tail
 * no view covers; here that is refused).  V = (H - Hw) / s + 1 <= 32 views, view v covers canvas rows [v s, v s + Hw).  The UNet runs
 * (cfg ? 2 : 1) * B * V rows of height Hw per step, row half * B * V + b * V + v for window v of sample b, unconditional half first:
 * prompt_embeds / prompt_mask (/ prompt_mask_host) hold that many rows in that order (repeat each sample's rows V times).
 * Per step and canvas element, over the views that cover its row in ascending order: d_v = the rule's `prev` of the plain update before
 * its noise term, from view v's guided output at the element's position in that window; r = (0 + d_.. + d_..) / count (fp32, IEEE division);
 * r += sigma * n when sigma > 0.  n is ONE draw per canvas element (noise[step][b, c, h, w], or Philox with the canvas position in the
 * counter) -- the fork's loop would average V independent draws and shrink the step noise; with sigma == 0 the update is the fork's.
 * V = 1 (H == Hw) computes tango_engine_denoise's bits.
 * Refused: TANGO_RULE_DPM_MULTISTEP (a per-view history has no reference behaviour), known_latents, a geometry that is no exact cover,
 * V > 32, a window_h that is no UNet height, and whatever tango_engine_denoise refuses.  There is no guidance table or rescale here. */
typedef struct tango_window_args {
  int32_t window_h;            /* Hw */
  int32_t stride;              /* s  */
} tango_window_args_t;
int tango_engine_denoise_windows(tango_engine_t* h, const tango_denoise_args_t* args, const tango_window_args_t* win, void* stream);
/* host-side query, no GPU needed: "" when tango_engine_denoise_windows accepts these arguments as far as its argument checks go (window_h
 * is only asked to be a multiple of 8: the heights of a configuration are checked by the call itself), else the message it fails with */
const char* tango_debug_denoise_windows_check(const tango_denoise_args_t* args, const tango_window_args_t* win);
/* latents [B, embed_dim, canvas_h, latent_w] -> mel [B, 1, 4 canvas_h, 64] (three VAE levels): the V = (canvas_h - window_h) / stride + 1 latent
 * windows of every sample go through the decoder at batch B * V and height window_h (a VAE height) in one run, and the decoded tiles are
 * cross-faded as tango_op_mel_tile_blend says.  All V tiles are decoded, overlaps included.  The same geometry rules as above. */
int tango_engine_vae_decode_tiled_h(tango_engine_t* h, const float* latents, float* mel, int batch, int canvas_h, int window_h, int stride,
                                    void* stream);

/* Seamless loops: the same windows on a RING in time.  The canvas args->latents [B, C_lat, H, latent_w] (H = args->latent_h > 0) is a ring
 * of H rows; V = H / s views, view v covers canvas rows (v s + y) mod H for y in [0, Hw).  1 <= s <= Hw <= H (a window never meets itself),
 * H % s == 0, V <= 32, Hw a UNet height.  H == Hw is a good call: V = Hw / s rotated views of the whole ring; H == Hw == s is one view
 * that does not wrap and computes tango_engine_denoise's bits.  The UNet batch, the row order of prompt_embeds / prompt_mask, the plan
 * and the captured steps a call replays are tango_engine_denoise_windows' of that shape.  Per step and canvas element of row h, with r = h % s: the n = ceil((Hw - r) / s) covering views are
 * v_k = (h / s - k) mod V, k = 0 .. n - 1, the element at local row y_k = r + k s of view v_k; they are accumulated in DESCENDING k (the view
 * that starts farthest below h first: for a row no view wraps over, the linear call's ascending order), acc = 0 + d_.. + d_..; acc / n;
 * + sigma * one draw per canvas element, exactly as above.  The order is relative to h, so the update commutes with a rotation of the ring
 * by a multiple of s: no row is special, the wrap point included.
 * Refused, each with a message of its own, in this order: TANGO_RULE_DPM_MULTISTEP, whatever tango_engine_denoise refuses, known_latents,
 * (a guidance table or rescale: there is none here), latent_h <= 0, H < Hw, H % s != 0, s outside [1, Hw], V > 32, no UNet height. */
int tango_engine_denoise_ring(tango_engine_t* h, const tango_denoise_args_t* args, const tango_window_args_t* win, void* stream);
/* host-side query, no GPU needed: "" when tango_engine_denoise_ring accepts these arguments as far as its argument checks go (window_h is
 * only asked to be a multiple of 8), else the message it fails with */
const char* tango_debug_denoise_ring_check(const tango_denoise_args_t* args, const tango_window_args_t* win);

/* Timed prompts: tango_engine_denoise_windows / tango_engine_denoise_ring with a TAPERED weight per window row (weighted MultiDiffusion,
 * "Mixture of Diffusers", Jimenez 2023).  Both calls already take one text row per window (row half * B * V + b * V + v), so windows of one
 * sample may run under different prompts; with equal weights every view would count in full up to the row where it ends and the canvas
 * would see a step in the mixture at every window edge.  view_weights is a HOST table of window_h floats, one weight per local window row,
 * shared by all views.  Per step and canvas element, over the covering views in exactly the unweighted call's order (ascending; on a ring,
 * the ring's order), with d_v the unweighted call's per-view value:
 *   acc = 0; wsum = 0;   t = w[y_v] * d_v; acc = acc + t; wsum = wsum + w[y_v];   r = acc / wsum (IEEE division);   + sigma * one draw
 * in fp32 without FMA contraction.  With all weights 1.0 the result is the unweighted call's, bit for bit; with one covering view and
 * w != 1, (w d) / w may differ from d in the last bit.  The profile of timed prompts is, with E = window_h - stride,
 * w[y] = min(1, (y + 0.5) / E) * min(1, (window_h - y - 0.5) / E) (1 when E == 0): tango_op_mel_ring_blend's.  Any table is taken.
 * Refused: whatever the unweighted call refuses, with the same messages under the prefix "denoise_windows_weighted: " /
 * "denoise_ring_weighted: "; then a NULL table, and a table with a non-finite entry or an entry <= 0.  The table is copied into a buffer
 * of the engine before the call returns to its loop; a weighted and an unweighted call of one shape share the UNet plan and replay
 * captured steps of their own. */
int tango_engine_denoise_windows_weighted(tango_engine_t* h, const tango_denoise_args_t* args, const tango_window_args_t* win,
                                          const float* view_weights /* HOST [window_h] */, void* stream);
int tango_engine_denoise_ring_weighted(tango_engine_t* h, const tango_denoise_args_t* args, const tango_window_args_t* win,
                                       const float* view_weights /* HOST [window_h] */, void* stream);
/* host-side queries, no GPU needed: "" when the weighted call accepts these arguments as far as its argument checks go, else its message */
const char* tango_debug_denoise_windows_weighted_check(const tango_denoise_args_t* args, const tango_window_args_t* win,
                                                       const float* view_weights);
const char* tango_debug_denoise_ring_weighted_check(const tango_denoise_args_t* args, const tango_window_args_t* win,
                                                    const float* view_weights);
/* ring latents [B, embed_dim, canvas_h, latent_w] -> mel [B, 1, 4 canvas_h, 64] on the same ring: the V = canvas_h / stride wrapping windows
 * go through the decoder at batch B * V and height window_h, and the tiles are cross-faded as tango_op_mel_ring_blend says. */
int tango_engine_vae_decode_ring_h(tango_engine_t* h, const float* latents, float* mel, int batch, int canvas_h, int window_h, int stride,
                                   void* stream);
/* mel [B, 1, T, num_mels] fp32 on a ring of T = mel_frames frames -> wav int16 [B, hop * T] (hop = the product of the upsample rates, 160):
 * the mel is padded circularly by Cx = tango_engine_vocoder_ring_context() frames on each side, the ordinary vocoder runs at T + 2 Cx
 * frames, and samples [hop Cx + 16, hop Cx + 16 + hop T) of each item (16 = half the 32 samples the vocoder makes beyond hop per frame) are
 * copied out.  The last sample joins the first as any two neighbours join. */
int tango_engine_vocode_ring(tango_engine_t* h, const float* mel, int16_t* wav, int batch, int mel_frames, int* n_samples, void* stream);
/* Cx: the vocoder's receptive field in mel frames on one side, from its configuration (kernels, dilations, rates), rounded up to a multiple of 4 */
int tango_engine_vocoder_ring_context(tango_engine_t* h);

/* one UNet call: sample [B2,C,H,W] fp32 NCHW, timestep, embeds [B2,L,d], mask [B2,L] -> out [B2,C,H,W] fp32 */
int tango_engine_unet_forward(tango_engine_t* h, const float* sample, int64_t timestep, const float* prompt_embeds,
                              const uint8_t* prompt_mask, float* out, int batch2, int text_len, void* stream);

/* UNet2DConditionModelMusic.forward (unet_2d_condition_music.py:536-757): as tango_engine_unet_forward plus the beat / chord
 * conditions [B2, beat_len | chord_len, d] fp32 and their bool masks (may be NULL) */
int tango_engine_unet_forward_music(tango_engine_t* h, const float* sample, int64_t timestep, const float* prompt_embeds,
                                    const uint8_t* prompt_mask, const float* beat_embeds, const uint8_t* beat_mask,
                                    const float* chord_embeds, const uint8_t* chord_mask, float* out, int batch2, int text_len,
                                    int beat_len, int chord_len, void* stream);

/* The *_h entry points below take the latent height of the call (the reference's duration_to_latent_t_size, audioldm/pipeline.py:94-95:
 * int(duration * 25.6)); 0 = tango_config_t.latent_h, which is what the entry points without the suffix pass.  The width is always
 * tango_config_t.latent_w.  UNet heights are multiples of 8 << (unet_levels - 1), VAE heights multiples of 8: an error otherwise. */
int tango_engine_unet_forward_h(tango_engine_t* h, const float* sample, int64_t timestep, const float* prompt_embeds,
                                const uint8_t* prompt_mask, float* out, int batch2, int text_len, int latent_h, void* stream);
int tango_engine_unet_forward_music_h(tango_engine_t* h, const float* sample, int64_t timestep, const float* prompt_embeds,
                                      const uint8_t* prompt_mask, const float* beat_embeds, const uint8_t* beat_mask,
                                      const float* chord_embeds, const uint8_t* chord_mask, float* out, int batch2, int text_len,
                                      int beat_len, int chord_len, int latent_h, void* stream);
/* latents [B,8,H,16] -> mel [B,1,4H,64]; mel [B,1,4H,64] -> moments [B,16,H,16] */
int tango_engine_vae_decode_h(tango_engine_t* h, const float* latents, float* mel, int batch, int latent_h, void* stream);
int tango_engine_vae_encode_h(tango_engine_t* h, const float* mel, float* moments, int batch, int latent_h, void* stream);
int tango_engine_profile_unet_h(tango_engine_t* h, int batch2, int text_len, int latent_h, char* report, int report_cap, void* stream);
int tango_engine_profile_vae_h(tango_engine_t* h, int batch, int latent_h, char* report, int report_cap, void* stream);

/* latents [B,8,256,16] fp32 -> mel [B,1,1024,64] fp32 */
int tango_engine_vae_decode(tango_engine_t* h, const float* latents, float* mel, int batch, void* stream);
/* AutoencoderKL.encode (autoencoder.py:52-58: Encoder.forward, modules.py:519-543, then quant_conv): mel [B, in_ch, 4H, 4W] fp32
 * NCHW (H, W = latent_h, latent_w for three levels) -> moments [B, 2*embed_dim, H, W] fp32 NCHW = [mean | logvar]; the posterior
 * (clamp, exp, sample: distributions.py:24-41) and scale_factor (autoencoder.py:126-135) are host-side code of the caller, or one
 * launch of tango_op_latent_encode below */
int tango_engine_vae_encode(tango_engine_t* h, const float* mel, float* moments, int batch, void* stream);
/* mel [B,1,T,num_mels] fp32 -> int16 [B, samples]; returns samples per item via *n_samples (may be NULL) */
int tango_engine_vocode(tango_engine_t* h, const float* mel, int16_t* wav, int batch, int mel_frames, int* n_samples, void* stream);
int tango_engine_vocoder_samples(tango_engine_t* h, int mel_frames);

/* T5 encoder forward (replaces text_encoder(input_ids, attention_mask)[0], models.py:139-141,279-281,291-293):
 * input_ids int64 [B, L] (device), attention_mask uint8 [B, L] (device, 1 = token, may be NULL), out fp32 [B, L, d_model] */
int tango_engine_encode_text(tango_engine_t* h, const int64_t* input_ids, const uint8_t* attention_mask, float* out, int batch,
                             int text_len, void* stream);

/* TacotronSTFT.mel_spectrogram (audioldm/audio/stft.py:164-186; callers tools/torch_tools.py:57-78): wav fp32 [B, n_samples]
 * in [-1, 1] (device) -> mel fp32 [B, n_mel, T] = log(clamp(mel_basis @ |STFT|, 1e-5)), log_magnitudes fp32 [B, n_fft/2+1, T]
 * (may be NULL), energy fp32 [B, T] (may be NULL); T = 1 + n_samples / hop (tango_engine_mel_frames), also returned via
 * *n_frames (may be NULL).  n_samples must exceed n_fft / 2 (reflect padding). */
int tango_engine_mel_frames(tango_engine_t* h, int n_samples);
int tango_engine_mel_spectrogram(tango_engine_t* h, const float* wav, float* mel, float* log_magnitudes, float* energy, int batch,
                                 int n_samples, int* n_frames, void* stream);

/* timing of the last denoise call's kernels, measured with HIP events on the launch stream */
int tango_engine_last_denoise_ms(tango_engine_t* h, float* total_ms, float* per_step_ms);
/* GFLOP one launch of the last denoise call's UNet step program EXECUTES (sum over its kernel groups; bench.py reports it beside
 * the reference's algorithmic 1606.36 GFLOP per prompt and step, which it undercuts wherever work was designed out: the single-key
 * rows of models.py:282-289, the step-invariant to_k / to_v of attention_processor.py:519-520).  No reference counterpart. */
int tango_engine_last_step_gflop(tango_engine_t* h, double* gflop);

/* diagnostic: eager run of one UNet step with HIP events around every kernel group; writes
 * "label<TAB>ms<TAB>GFLOP" lines into `report` (truncated to report_cap). */
/* Plan cache.  The engine keeps one workspace slab + launch program ("plan") per call shape: UNet (batch, text / beat / chord
 * lengths, single-key prefix), VAE / vocoder (batch, frames), text encoder (batch, length), STFT (batch, samples).  All of them
 * share one byte budget (default 64 GiB, or TANGO_PLAN_BUDGET_MB); when a new plan does not fit, least recently used plans are
 * freed first (hipFree: synchronises the device).  The reference has no counterpart: tango.py:51-64 just re-runs PyTorch eagerly. */
int tango_engine_set_plan_budget(tango_engine_t* h, uint64_t bytes);
int tango_engine_plan_stats(tango_engine_t* h, uint64_t* bytes_in_use, int* plans);
/* diagnostic: capacity in floats of the multistep history ring (3 * B * C * H * W of the largest TANGO_RULE_DPM_MULTISTEP call so far; 0 before) */
int tango_engine_ring_elems(tango_engine_t* h, uint64_t* elems);
/* frees every cached plan now (the next call of each shape rebuilds its plan); also what a measurement tool calls after
 * tango_tuning_reload() so that build-time routing decisions are taken again */
int tango_engine_drop_plans(tango_engine_t* h);

int tango_engine_profile_unet(tango_engine_t* h, int batch2, int text_len, char* report, int report_cap, void* stream);
/* the same per-op table ("label\tms\tGFLOP" lines, HIP events around every op of the eager plan) for the two stages that follow the
 * denoise loop in every pass: the mel-VAE decoder (audioldm/variational_autoencoder/modules.py:546-683, autoencoder.py:116-124) for
 * `batch` latents, and HiFi-GAN (audioldm/hifigan/models.py:96-165) for `batch` mels of `frames` frames.  Measurement tools only. */
int tango_engine_profile_vae(tango_engine_t* h, int batch, char* report, int report_cap, void* stream);
int tango_engine_profile_vocoder(tango_engine_t* h, int batch, int frames, char* report, int report_cap, void* stream);
/* measurement tools only: re-read the TANGO_* dispatch switches (csrc/tuning.h) from the environment, so that one process can
 * time several arms of an A/B back to back (tools/profile_unet_ops.py --ab).  No reference counterpart. */
void tango_tuning_reload(void);
/* host-side query, no GPU needed: the kernel family the GEMM dispatcher (csrc/gemm.hip gemm_route) picks for the 16-bit linear
 * y[M,N] = epi(x[M,K] W[N,K]^T): "wide", "wide+pers", "duo", "stream", "dma", "tile", "tile+splitk", "wide+xstats" (GEGLU with external
 * LayerNorm statistics), or "layernorm+<route>" when no kernel folds the LayerNorm for that shape.  dtype 1 = fp16, 2 = bf16.
 * tests/test_routing.py pins the measured routing rules of the UNet's shapes with it.  No reference counterpart. */
const char* tango_debug_linear_route(int dtype, int M, int N, int K, int geglu, int ln_fold, int residual, int vt);
/* the GroupNorm kernel form tango_op_groupnorm runs for this shape under the current switches: "slab", "coop" (cooperative single launch), "group" (one
   workgroup per (sample, group)), "two" (statistics + apply launches); "" = refused.  Asks the device for the cooperative kernel's occupancy. */
const char* tango_debug_groupnorm_form(int dtype, int B, int C, int HW, int groups);
/* host-side query, no GPU needed: the attention kernel tango_op_attention[_ex] and the engine run for this problem under the current switches, as
 * "qb<query blocks per wave>:<form> <grid x>x<y>x<z>", e.g. "qb2:msum+kdma+vdma 32x5x32"; forms: plain, masked, posbias, msum, defer, msum+defer, msum+kdma,
 * msum+kdma+vdma, f8, f8+msum, x8.  Arguments the launch refuses answer its message instead.  masked / pos_bias: a key-mask bias / a relative position
 * bias is given; fp8_pv 0 | 1 | 2 and vt_perm as in tango_op_attention_ex's flags.  dtype 0 = fp32, 1 = fp16, 2 = bf16.  tests/test_attention_routes.py */
const char* tango_debug_attention_route(int dtype, int B, int heads, int Sq, int Skv, int masked, int pos_bias, int fp8_pv, int vt_perm);
/* the same for buffers with the given pitches in elements (tango_debug_attention_route asks ldq = ldk = ldo = heads * 64, ldvt = round8(Skv)): the
 * engine's self-attention reads q | k from one buffer of pitch 2 * heads * 64, its cross-attention q from that buffer and k at pitch heads * 64.  The
 * answer depends on the pitches only through the ld-alignment refusal (16-byte q / k / v^T rows, 8-byte output rows) */
const char* tango_debug_attention_route_ld(int dtype, int B, int heads, int Sq, int Skv, int masked, int pos_bias, int fp8_pv, int vt_perm, int ldq,
                                           int ldk, int ldvt, int ldo);

/* ---- per-operator entry points (parity tests; fp32 reference-layout tensors on device) ---- */
int tango_op_conv2d(int dtype, const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W,
                    int Cout, int stride, int upsample, void* stream);
/* nearest x2 upsampling + 3x3 / pad 1 conv of a 16-bit engine (x [B][Cin][H][W] -> out [B][Cout][2H][2W]); bias2 [Cout] (may be null) is
 * added like the per-step bias of the UNet.  phases = 1: as four 2x2-tap phase convolutions on the source grid (an error where that form
 * does not take the problem), 0: the nine-tap gather form.  tango_op_conv2d(..., upsample = 1) picks as the engine does. */
int tango_op_conv2d_ups(int dtype, const float* x, const float* w, const float* bias, const float* bias2, float* out, int B, int Cin,
                        int H, int W, int Cout, int phases, void* stream);
/* the summed phase weights of such a conv: w fp32 OIHW [Cout][Cin][3][3] -> out, 16-bit engine dtype, [4 phases][Cout][2x2 taps][Cin] */
int tango_op_pack_ups_phase(int dtype, const float* w, void* out, int Cout, int Cin, void* stream);
int tango_op_linear(int dtype, const float* x, const float* w, const float* bias, const float* residual, float* out, int M,
                    int N, int K, int a_act, int e_act, int geglu, void* stream);
int tango_op_linear_ln(int dtype, const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                       const float* residual, float* out, int M, int N, int K, int geglu, float eps, void* stream);
/* out[M,N] = x[M,K] W^T (+ bias) (+ bias2[step]) (+ residual) with the epilogue arms only the engine's plan builders set (tests/
 * test_gemm_engine_arms_gpu.py); split-K as the engine applies it.  All tensors fp32 on the device.
 *   bias2 [steps][N] or NULL: the per-step bias table; `step` goes into a device int the kernels read.  step = -1: no step pointer (row 0).
 *   rowvec [ceil(rowvec_rows / rowvec_per)][N] or NULL: rows m < rowvec_rows also get rowvec[m / rowvec_per] and are written to out_lo, not out.
 *   wb_rows != 0: w holds M / wb_rows matrices [N][K] back to back, rows [s wb_rows, (s + 1) wb_rows) multiply with the s-th.  The weight
 *   rows are dense inside (row stride Kp = K, so wb_stride = N K): K must be a whole number of 16-byte vectors or the launch is refused.
 *   pad (0 or a multiple of 8): the activation, residual and out rows are pitched to K + pad / N + pad elements inside; out is fp32
 *   [M][N + pad] and out_lo (required with rowvec) fp32 [M][N + (pad ? pad + 8 : 0)].  Both are copied INTO the launch's output buffers first,
 *   pitch columns included, and copied back whole: what the launch did not write comes back as the caller left it (rounded to the dtype).
 *   plan (may be NULL): receives the plan name of the launch ("wide", "wide+pers", "duo", "tile", "tile+splitk", "dma", ...). */
int tango_op_linear_ex(int dtype, const float* x, const float* w, const float* bias, const float* bias2, int steps, int step,
                       const float* residual, const float* rowvec, int rowvec_rows, int rowvec_per, int wb_rows, int pad, float* out,
                       float* out_lo, int M, int N, int K, char* plan, int plan_cap, void* stream);
/* host-side query, no GPU needed: "" when launch_gemm accepts the problem tango_op_linear_ex builds for these arguments (the int flags say which
 * pointers are set; geglu puts the GEGLU epilogue on top), else the message it fails with; plan as above.  tests/test_gemm_refusals.py */
const char* tango_debug_linear_ex_check(int dtype, int M, int N, int K, int residual, int bias2, int rowvec, int rowvec_rows, int rowvec_per,
                                        int out_lo, int wb_rows, int pad, int geglu, char* plan, int plan_cap);
/* conv1 of a ResNet block: 3x3 / stride 1 / pad 1 conv + bias + bias2[step] (the time-embedding table [steps][Cout], step in a device int)
 * (+ residual [B][Cout][H][W] or NULL); plan as above */
int tango_op_conv2d_temb(int dtype, const float* x, const float* w, const float* bias, const float* bias2, int steps, int step,
                         const float* residual, float* out, int B, int Cin, int H, int W, int Cout, char* plan, int plan_cap, void* stream);
/* tango_op_conv2d_ups with bias2 as such a table */
int tango_op_conv2d_ups_temb(int dtype, const float* x, const float* w, const float* bias, const float* bias2, int steps, int step, float* out,
                             int B, int Cin, int H, int W, int Cout, int phases, char* plan, int plan_cap, void* stream);
/* fused self-attention projection as the engine runs it (reference: diffusers attention_processor.py Attention.to_q/to_k/to_v on
   LayerNorm(x), transformer_2d BasicTransformerBlock.norm1): q | k row-major into out_qk [B*S, 2C], v TRANSPOSED into out_vt
   [B][C][S]; gamma == NULL skips the LayerNorm */
int tango_op_linear_qkv(int dtype, const float* x, const float* w, const float* gamma, const float* beta, float* out_qk,
                        float* out_vt, int B, int S, int C, int K, float eps, void* stream);
/* the same with the tokens of every block of 32 of out_vt in the attention kernel's fragment order when vt_perm = 1 (position 8 g + 4 hi + r
   holds token 16 hi + 4 g + r: what tango_op_attention's LDS-DMA form reads; 16-bit engines, S % 32 == 0) */
int tango_op_linear_qkv_perm(int dtype, const float* x, const float* w, const float* gamma, const float* beta, float* out_qk,
                             float* out_vt, int B, int S, int C, int K, float eps, int vt_perm, void* stream);
/* the level-0 feed-forward of BasicTransformerBlock with its LayerNorm and residual (reference: diffusers attention.py:326-335 norm3 -> ff ->
   + hidden_states, :338-387 FeedForward, :412-433 GEGLU): out [M, C] = x + W2 GEGLU(W1 LayerNorm(x) + b1) + b2, w1 [2H, C] in the reference
   row order (value rows, then gate rows), w2 [C, H].  mode 0 = ONE launch (csrc/ff_fused.hip; C = 320, H = 1280, M % 128 == 0, 16-bit),
   mode 1 = the engine's two-GEMM route.  reps > 0 with ms_out != NULL: mean milliseconds of `reps` repeats (HIP events) -- same-process A/B. */
int tango_op_ff_fused(int dtype, const float* x, const float* w1, const float* b1, const float* gamma, const float* beta, const float* w2,
                      const float* b2, float* out, int M, int C, int H, float eps, int mode, int reps, float* ms_out, void* stream);
/* as tango_op_linear_qkv with LayerNorm (K = C): mode 0 = the activation-stationary kernel of the level-0 sites (csrc/ff_fused.hip
   qkv_stat_kernel: C = 320, (B * S) % 256 == 0, S % 256 == 0, 16-bit), mode 1 = the GEMM route; reps / ms_out as tango_op_ff_fused */
int tango_op_qkv_stat(int dtype, const float* x, const float* w, const float* gamma, const float* beta, float* out_qk, float* out_vt, int B,
                      int S, int C, float eps, int mode, int reps, float* ms_out, void* stream);
int tango_op_conv1d(int dtype, const float* x, const float* w, const float* bias, const float* residual, float* out, int B,
                    int Cin, int L, int Cout, int k, int dilation, int a_act, float a_slope, int e_act, float e_slope, void* stream);
int tango_op_conv_transpose1d(int dtype, const float* x, const float* w, const float* bias, float* out, int B, int Cin, int L,
                              int Cout, int k, int stride, int padding, int a_act, float a_slope, void* stream);
/* ---- the gather-GEMM modes and epilogues only the mel-VAE (audioldm/variational_autoencoder/modules.py) and HiFi-GAN (audioldm/hifigan/models.py)
 * plans use, and the elementwise kernels around them (tests/test_vae_voc_ops_gpu.py) ---- */
/* 3x3 conv, stride 1 | 2, no upsampling.  pad 1: F.conv2d(x, w, b, stride, padding=1); pad 0: F.conv2d(F.pad(x, (0,1,0,1)), w, b, stride), the
 * VAE Downsample (modules.py:87-91).  residual [B][Cout][Ho][Wo] or NULL is added after the epilogue activation e_act (0 none, 1 SiLU,
 * 2 leaky-ReLU with e_slope, 4 tanh).  out_f32: the GEMM itself writes fp32 rows of Cout channels, as the VAE plan does for conv_out */
int tango_op_conv2d_ex(int dtype, const float* x, const float* w, const float* bias, const float* residual, float* out, int B, int Cin, int H,
                       int W, int Cout, int stride, int pad, int e_act, float e_slope, int out_f32, void* stream);
/* out[b] = alpha * A[b] W[b]^T + bias, fp32 [batch][M][N]: GemmParams::batch as Builder::vae_attn uses it.  a [batch][M][lda] (a_shared: [M][lda],
 * one A for every batch item, stride 0); w [batch][N][ldw], or NULL: W[b] is the view of a[b] that starts w_col_off columns in (N == M,
 * ldw == lda: the k half of a q | k buffer).  bias [N], or [M] indexed by output row when bias_rows; may be NULL */
int tango_op_gemm_batched(int dtype, const float* a, const float* w, const float* bias, float* out, int batch, int M, int N, int K, int lda,
                          int ldw, int w_col_off, int a_shared, float alpha, int bias_rows, void* stream);
/* out = softmax(x * scale) over each row of x [rows][cols], computed in place on the engine-dtype copy (csrc/norm.hip softmax_rows_kernel) */
int tango_op_softmax_rows(int dtype, const float* x, float* out, int rows, int cols, float scale, void* stream);
/* HiFi-GAN conv_post + tanh + the int16 conversion of hifigan/utilities.py:81 in the GEMM epilogue (EPI_I16, out_scale 32768: C truncation,
 * int16 wrap): out int16 DEVICE, channels-last [B][L][Cout] (Cout = 1: [B][L]) */
int tango_op_conv1d_i16(int dtype, const float* x, const float* w, const float* bias, int16_t* out, int B, int Cin, int L, int Cout, int k,
                        int dilation, void* stream);
/* out = act(((a + b) + c) * scale) on n engine-dtype elements (the resblock average of hifigan/models.py:153-161); n must be a multiple of
 * the 16-byte vector: an error otherwise */
int tango_op_avg3_act(int dtype, const float* a, const float* b, const float* c, float* out, int64_t n, float scale, int act, float slope,
                      void* stream);
/* 1x1 conv of scale * x, x fp32 [B][Cin][HW] (Cin <= 16), into engine-dtype channels-last rows of ld channels; out fp32 [B*HW][Cout]
 * (post_quant_conv of z / scale_factor, autoencoder.py:121) */
int tango_op_pointwise_small(int dtype, const float* x, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int HW, int ld,
                             float scale, void* stream);
/* 1x1 conv of fp32 channels-last rows x [B*HW][ld] (first Cin <= 32 channels) into fp32 NCHW out [B][Cout][HW] (quant_conv, autoencoder.py:56) */
int tango_op_pointwise_out_nchw(const float* x, int ld, const float* w, const float* bias, float* out, int B, int Cin, int Cout, int HW,
                                void* stream);
/* host-side queries beside tango_debug_linear_route, no GPU needed: the kernel family that takes the problem tango_op_conv2d[_ex] builds for
 * these arguments -- "tile", "dma", "conv_wide", "conv_halo", "wide", "duo", "stream" -- with "+splitk" when the wrappers' split-K policy
 * splits it (*splitk, if not NULL, receives the factor; 1 = unsplit) and "+phase" for an upsampler conv in the four-phase form */
const char* tango_debug_conv2d_route(int dtype, int B, int Cin, int H, int W, int Cout, int stride, int ups, int pad, int residual, int e_act,
                                     int out_f32, int* splitk);
/* ... for a conv1d or transposed-conv1d phase: rows_pb output rows per batch item, row q reads inputs q + in_off + tap * tap_step of L and
 * writes row q * out_mul + out_off.  tango_op_conv1d(k, dilation d) is taps = k, tap_step = d, in_off = -d (k - 1) / 2, rows_pb = L, out_mul 1 */
const char* tango_debug_conv1d_route(int dtype, int B, int Cin, int L, int Cout, int taps, int tap_step, int in_off, int rows_pb, int out_mul,
                                     int out_off, int a_act, int residual, int e_act, int* splitk);
/* phase r of the decomposition tango_op_conv_transpose1d runs: geom6 = {taps, tap_step, in_off, rows_pb, out_mul, out_off} for the query above;
 * returns 0 when the phase is empty */
int tango_debug_conv_transpose1d_phase(int B, int Cin, int L, int Cout, int k, int stride, int padding, int r, int* geom6);
int tango_op_groupnorm(int dtype, const float* x, const float* gamma, const float* beta, float* out, int B, int C, int HW,
                       int groups, float eps, int act, void* stream);
int tango_op_layernorm(int dtype, const float* x, const float* gamma, const float* beta, float* out, int rows, int C, float eps,
                       void* stream);
int tango_op_attention(int dtype, const float* q, const float* k, const float* v, const float* bias, float* out, int B, int heads,
                       int Sq, int Skv, float scale, void* stream);
/* as tango_op_attention; flags bit 0: P.V on the fp8 MFMA (16-bit dtypes, no bias, Skv % 64 == 0); bit 1 (with bit 0): on the MX
 * instruction, 128 keys per MFMA (Skv % 128 == 0); bit 2: the rows of v are given in the kernel's fragment order inside every block of
 * 32 keys (row 8 g + 4 hi + r of a block holds key 16 hi + 4 g + r) -- the op's V^T is then the permuted one the engine's producers write
 * and both tiles travel by LDS-DMA (unmasked 16-bit problems with Sq > 512, Skv % 64 == 0; refused otherwise) */
int tango_op_attention_ex(int dtype, const float* q, const float* k, const float* v, const float* bias, float* out, int B, int heads,
                          int Sq, int Skv, float scale, int flags, void* stream);
/* as tango_op_attention_ex on the memory layouts the engine hands the kernel instead of the dense one.  pos_bias: fp32 [heads][Sq][Skv] on the
 * device or NULL, passed as it is (the text encoder's relative position bias; not with an fp8 flag).  k_col0 >= 0 (needs Sq == Skv and
 * ldk == ldq): q and k are staged into ONE [B*S][ldq] buffer, q in columns [0, C) and k in [k_col0, k_col0 + C), C = heads * 64, as
 * Builder::transformer and build_t5 slice their projection; k_col0 = -1: two buffers of pitches ldq and ldk.  ldvt >= round8(Skv) is the
 * pitch of the staged V^T; the output buffer is [B*Sq][ldo] with the result in columns [o_col0, o_col0 + C).  pad_value (finite), rounded
 * to the dtype, fills every staged element that is not payload -- the pitch columns of q and k, the V^T columns >= Skv and the whole output
 * buffer before the launch -- and out, fp32 [B*Sq][ldo], receives the whole pitched output buffer, pads included.  Refused before any launch:
 * a non-finite pad_value, a pitch below C (ldvt below round8(Skv)) or beyond 65536, a column range outside its row, q / k / v^T bases that are
 * not 16-byte or an output base that is not 8-byte aligned (the column offsets are in elements), pos_bias with an fp8 flag. */
int tango_op_attention_view(int dtype, const float* q, const float* k, const float* v, const float* bias, const float* pos_bias, float* out,
                            int B, int heads, int Sq, int Skv, float scale, int flags, int ldq, int ldk, int k_col0, int ldvt, int ldo,
                            int o_col0, float pad_value, void* stream);
/* fused cross-attention block of BasicTransformerBlock (diffusers attention.py:312-323: attn2(norm2(x), text, mask) + x) as the engine
   runs it at level 0 (C = 320, 5 heads, 64 text tokens): x [B*HW, 320]; wq / wo [320, 320] Linear weights (to_q has no bias);
   k, v [B*L, 320] = to_k / to_v of the text; bias [B, L] additive or NULL */
int tango_op_xattn_block(int dtype, const float* x, const float* gamma, const float* beta, const float* wq, const float* k, const float* v,
                         const float* bias, const float* wo, const float* bo, float* out, int B, int HW, int L, float eps, void* stream);
/* The four tango_op_sched_* hooks below are one implementation and refuse what tango_engine_denoise refuses for the row of their step
 * (unknown rule, coefficient width against the rule, step noise or clip with the multistep rule, table column 11 not 0 / 1, a row
 * order the loop index does not allow, masked arguments that do not go together, rescale outside [0, 1], guidance entries that are
 * negative or not finite), besides sizes <= 0 and missing latents / model_out_nchw / coef. */

/* one fused CFG + DDPM (rule 0) / DDIM (rule 1) step on caller-owned buffers: latents [B, C, HW] fp32 in/out, model_out_nchw
 * [B2, C, HW] fp32, noise DEVICE [B, C, HW] or NULL (Philox, seed 0), coef8 HOST [8] (the row of this step), clip / clip_range as
 * tango_denoise_args_t.clip_sample / clip_sample_range.  Synchronises. */
int tango_op_sched_step(float* latents, const float* model_out_nchw, const float* noise, const float* coef8, int B, int C, int HW,
                        int cfg, float guidance, int pred_type, int rule, int clip, float clip_range, void* stream);

/* one windowed update (tango_engine_denoise_windows) at loop index `step` on caller-owned fp32 buffers: latents [B, C, H, W] the canvas,
 * in/out; model_out_nchw [B2 * V, C, Hw, W] the UNet output of the window batch (B2 = 2B, [uncond; cond], when cfg; row b * V + v of a
 * half); noise DEVICE [B, C, H, W], this step's canvas noise, or NULL (Philox: seed, sample_offset, `step` and the canvas position); coef8
 * HOST [8], the row of this step.  Refuses what tango_engine_denoise_windows refuses.  Synchronises. */
int tango_op_sched_windows(float* latents, const float* model_out_nchw, const float* noise, const float* coef8, int B, int C, int H, int W,
                           int Hw, int s, int cfg, float guidance, int pred_type, int rule, int clip, float clip_range, uint64_t seed,
                           int sample_offset, int step, void* stream);
/* cross-fade of decoded tiles (the fork's tiled VAE decode, mustango/diffusers/src/diffusers/models/autoencoder_kl.py:198-201, 255-296): tiles
 * DEVICE fp32 [B * V, 1, Hw4, F], tile t holding output rows [t s4, t s4 + Hw4) -> out DEVICE fp32 [B, 1, (V - 1) s4 + Hw4, F].  With
 * E = Hw4 - s4 the weight of tile t at its local row y is min(1, (y + 0.5) / E) if t > 0, times min(1, (Hw4 - y - 0.5) / E) if t < V - 1
 * (both 1 when E == 0); out[r] = (sum_t w_t tile_t) / (sum_t w_t) over the covering tiles in ascending order, fp32.  For s4 >= Hw4 / 2 two
 * overlapping weights sum to 1: blend_v's ramp at half-pixel centres.  1 <= s4 <= Hw4, V <= 32.  Synchronises. */
int tango_op_mel_tile_blend(const float* tiles, float* out, int B, int V, int Hw4, int F, int s4, void* stream);
/* tango_op_sched_windows on a ring (tango_engine_denoise_ring): latents [B, C, H, W] the ring, model_out_nchw [B2 * (H / s), C, Hw, W].
 * Refuses what tango_engine_denoise_ring refuses.  Synchronises. */
int tango_op_sched_ring(float* latents, const float* model_out_nchw, const float* noise, const float* coef8, int B, int C, int H, int W,
                        int Hw, int s, int cfg, float guidance, int pred_type, int rule, int clip, float clip_range, uint64_t seed,
                        int sample_offset, int step, void* stream);
/* tango_op_sched_windows / tango_op_sched_ring with view_weights HOST [Hw] (tango_engine_denoise_windows_weighted): the weighted mean of
 * the views.  They refuse what those refuse, then a NULL or bad table.  Synchronise. */
int tango_op_sched_windows_weighted(float* latents, const float* model_out_nchw, const float* noise, const float* coef8,
                                    const float* view_weights, int B, int C, int H, int W, int Hw, int s, int cfg, float guidance, int pred_type,
                                    int rule, int clip, float clip_range, uint64_t seed, int sample_offset, int step, void* stream);
int tango_op_sched_ring_weighted(float* latents, const float* model_out_nchw, const float* noise, const float* coef8,
                                 const float* view_weights, int B, int C, int H, int W, int Hw, int s, int cfg, float guidance, int pred_type,
                                 int rule, int clip, float clip_range, uint64_t seed, int sample_offset, int step, void* stream);
/* cross-fade of decoded tiles on a ring: tiles DEVICE fp32 [B * V, 1, Hw4, F], tile t holding ring rows (t s4 + y) mod (V s4) -> out DEVICE
 * fp32 [B, 1, V s4, F].  Every tile has a predecessor and a successor: with E = Hw4 - s4 the weight at local row y is
 * min(1, (y + 0.5) / E) * min(1, (Hw4 - y - 0.5) / E) (1 when E == 0); out[r] = (sum w tile) / (sum w) over the covering tiles in the ring
 * update's order, fp32.  1 <= s4 <= Hw4 <= V s4, V <= 32.  Synchronises. */
int tango_op_mel_ring_blend(const float* tiles, float* out, int B, int V, int Hw4, int F, int s4, void* stream);
/* circular padding: mel DEVICE fp32 [B, T, F] -> out DEVICE fp32 [B, T + 2 ctx, F], out frame j = mel frame (j - ctx) mod T.  Synchronises. */
int tango_op_mel_ring_pad(const float* mel, float* out, int B, int T, int F, int ctx, void* stream);

/* one fused CFG + multistep DPM-Solver step (TANGO_RULE_DPM_MULTISTEP) at loop index `step` on caller-owned buffers: latents
 * [B, C, HW] fp32 in/out, model_out_nchw [B2, C, HW] fp32 (B2 = 2B, [uncond; cond], when cfg), ring DEVICE [3][B][C][HW] fp32
 * (the converted outputs of steps step - 1 and step - 2 in slots (step + 2) % 3 and (step + 1) % 3; this step's goes to
 * step % 3), coef16 HOST [step + 1][16] (the table up to this step), algo 0 DPM-Solver++ / 1 DPM-Solver (the argument
 * decides, whatever column 11 of the table says; column 11 of row 0 must still be 0 or 1, and the order column exactly 1, 2 or 3).
 * Synchronises. */
int tango_op_sched_multistep(float* latents, const float* model_out_nchw, float* ring, const float* coef16, int step, int B, int C,
                             int HW, int cfg, float guidance, int pred_type, int algo, void* stream);

/* the N(0,1) values the denoise loop's device Philox generator injects at loop index `step` for global samples
 * [sample_offset, sample_offset + B): out fp32 [B, C, HW] (replaces randn_tensor inside DDPMScheduler.step,
 * mustango/diffusers/src/diffusers/schedulers/scheduling_ddpm.py:331-338, for throughput runs) */
int tango_op_philox_normal(float* out, int B, int C, int HW, int step, uint64_t seed, int sample_offset, void* stream);

/* loop index `step` of a masked (inpainting) loop on caller-owned buffers, fp32: at step 0 the pre-loop blend of latents with the
 * known latents first, then the fused CFG + update of `rule` (TANGO_RULE_*), then -- when step + 1 < num_steps -- the blend for loop
 * index step + 1 (tango_denoise_args_t.known_latents).  latents [B, C, HW] in/out, model_out_nchw [B2, C, HW], noise DEVICE
 * [num_steps][B, C, HW] step noise or NULL (Philox; must be NULL for the multistep rule), ring DEVICE [3][B][C][HW] (multistep rule,
 * as tango_op_sched_multistep; else may be NULL), coef HOST [num_steps][coef_width] (8 or 16), known / mask DEVICE [B, C, HW] /
 * [B, HW], blend_coef HOST [num_steps][2], blend_noise DEVICE [num_steps][B, C, HW] or NULL (Philox).  Synchronises. */
int tango_op_sched_masked(float* latents, const float* model_out_nchw, const float* noise, float* ring, const float* coef, int coef_width,
                          int step, int num_steps, const float* known_latents, const float* latent_mask, const float* blend_coef,
                          const float* blend_noise, uint64_t seed, int sample_offset, int B, int C, int HW, int cfg, float guidance,
                          int pred_type, int rule, void* stream);

/* tango_op_sched_masked's arguments, for every rule, masked (known_latents, latent_mask and blend_coef set) or not (all three and
 * blend_noise NULL), through the guided kernels: guidance_row HOST [B] is the scale of each sample at this step (cfg must be 1; the
 * scalar `guidance` is not read), rescale = phi as in tango_guidance_args_t, scale_out HOST [B] or NULL receives the s_b the kernel
 * used (1.0 everywhere when rescale == 0: no statistics are taken).  Synchronises. */
int tango_op_sched_guided(float* latents, const float* model_out_nchw, const float* noise, float* ring, const float* coef, int coef_width,
                          int step, int num_steps, const float* known_latents, const float* latent_mask, const float* blend_coef,
                          const float* blend_noise, uint64_t seed, int sample_offset, int B, int C, int HW, int cfg, float guidance,
                          int pred_type, int rule, const float* guidance_row, float rescale, float* scale_out, void* stream);

/* the N(0,1) values the masked loop's device Philox generator uses as the blend noise n_step of loop index `step` (the step noise's
 * counter with bit 31 of the step word set): out fp32 [B, C, HW] */
int tango_op_philox_normal_blend(float* out, int B, int C, int HW, int step, uint64_t seed, int sample_offset, void* stream);

/* Fused latent encode of audio-to-audio editing (AudioLDM style_transfer, audioldm/pipeline.py:145-247): VAE moments -> the latents a
 * truncated denoise loop starts from, in one launch, ASYNCHRONOUS on `stream` (no synchronise, no scratch).  For sample b:
 *   lv = clamp(logvar, -30, 20); z = mean + exp(0.5 * lv) * eps     distributions.py:24-41 (posterior_mode 1: z = mean)
 *   z  = scale * z                                                  autoencoder.py:126-135
 *   if max over the sample of |z| > clip_trigger: z = clamp(z, -clip_range, clip_range)        pipeline.py:209-210 (1e2, 10)
 *   xt = sa * z + sb * n                                            latent_diffusion/ddim.py:259-262 == the fork's add_noise
 * each line in that multiply / add order without FMA contraction; exp is the only inexact operation.
 * The clip condition is per sample: the reference takes the maximum over the whole tensor, but its only caller repeats one clip
 * `batchsize` times, where the two agree -- and per sample the result does not depend on how a batch is split.
 * moments: device fp32 [moments_batch, 2C, HW] = [mean | logvar]; moments_batch is B, or 1 (one clip fans out to B samples).
 * xt_out: device fp32 [B, C, HW].  z0_out: the same shape or NULL: the clean scaled (clipped) latents, a masked edit's known_latents.
 * eps, noise: device fp32 [B, C, HW], or NULL -> device Philox with the denoise loop's key (seed) and counter layout
 *   (hw, c / 4, sample_offset + b, word) on two streams of their own, word = 0x40000000 | 0 (eps) and 0x40000000 | 1 (noise):
 *   step noise has bits 31 and 30 of the word clear, blend noise has bit 31 set, so the four streams are disjoint while a loop has
 *   fewer than 2^30 steps.  A Philox stream needs C % 4 == 0.  Any HW.
 *   With noise NULL and sb == 0 (the posterior alone) no n is drawn: xt = sa * z, and C is not constrained by that stream.
 * Errors: moments_batch not 1 or B, C % 4 != 0 with Philox, non-positive sizes. */
int tango_op_latent_encode(const float* moments, int moments_batch, float* z0_out, float* xt_out, const float* eps, const float* noise,
                           int B, int C, int HW, float scale, float clip_trigger, float clip_range, float sa, float sb,
                           int posterior_mode, uint64_t seed, int sample_offset, void* stream);

/* the N(0,1) values tango_op_latent_encode's device Philox generator draws for global samples [sample_offset, sample_offset + B):
 * which = 0 the posterior's eps, 1 the forward noise n; out fp32 [B, C, HW].  Synchronises.
 * Errors: out NULL, non-positive sizes, B * C * HW >= 2^31, which not 0 or 1. */
int tango_op_philox_normal_encode(float* out, int B, int C, int HW, int which, uint64_t seed, int sample_offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TANGO_ENGINE_H */

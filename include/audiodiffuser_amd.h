/* C ABI of libadf_hip.so -- the MI355X (gfx950) implementation of AudioDiffuser's EDM sampling hot path.
 *
 * What each entry point replaces in the reference (paths relative to the reference repo):
 *   adf_create / adf_load_weight   <- UNet1dBase.__init__ + Lightning strict state_dict load
 *                                     (src/models/backbones/unet1d.py:818-862, src/eval.py:73)
 *   adf_net_forward                <- UNet1dBase.forward            (src/models/backbones/unet1d.py:864-893, :771-816)
 *   adf_denoise                    <- Diffusion.denoise_fn + EluDiffusion.get_scale_weights + clip
 *                                     (src/models/components/diffusion.py:32-63, :232-241; components/utils.py:20-22)
 *   adf_sampler_run                <- EDMSampler.forward / EDMAlphaSampler.forward / DPMSampler.forward (multistep) /
 *                                     DPM2Sampler.forward (src/models/components/sampler_edm.py:371-397, :284-300,
 *                                     :710-768, :470-493), ADPM2Sampler.forward (stochastic_sampler_edm.py:85-100), UniPCSampler.forward (:996-1053)
 *   adf_sampler_run_table          <- VESampler.forward / VPSampler.forward (sampler_edm.py:99-123, :201-227), VSampler.forward / VEulerSampler.forward
 *                                     (src/models/components/sampler_vobj.py:176-194, :92-109): one generic loop over a host table of per-step records
 *   adf_sampler_run_program        <- sampler_vobj.DPMSampler.forward / UniPCSampler.forward (src/models/components/sampler_vobj.py:389-499, :670-732):
 *                                     one generic straight-line program over a small register file of state buffers, for linear multistep methods;
 *                                     with it all ten files under configs/experiment/sc09_inference/ run through this library
 *   the call site all of them sit behind: src/models/diffunet_complex_module.py:86-89
 *   adf_adm_create                 <- UNetModel.__init__ (src/models/backbones/unet2d_oai.py:410-601); adf_net_forward on that handle
 *                                     <- UNetModel.forward (:603-634)
 *   adf_wavenet_create             <- WaveNetNoise.__init__ (src/models/backbones/wavenet.py:153-167); the handle it returns goes
 *                                     through the same entry points: adf_load_weight (the module's state_dict keys, incl. the
 *                                     custom WeightNorm's weight_g / weight_v, wavenet.py:15-55), adf_net_forward
 *                                     <- WaveNetNoise.forward (wavenet.py:169-180), adf_denoise / adf_sampler_run as above
 *   adf_unet2d_create              <- UNet2dBase.__init__ (src/models/backbones/unet2d.py:622-876); adf_net_forward on that handle
 *                                     <- UNet2dBase.forward (:879-972)
 *   adf_dac_create / adf_dac_forward <- dac.py::Decoder (src/models/backbones/dac/dac.py:108-137), dac.py::Encoder (:57-84), FineTuneAutoencoder.decode (dac_vae.py:69-71)
 *   adf_dac_encode                 <- FineTuneAutoencoder.encode(x, is_train=False) (dac_vae.py:50-67)
 *   adf_dit_create                 <- DiT.__init__ (src/models/backbones/dit.py:282-326); adf_net_forward on that handle <- DiT.forward (:382-429)
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; adf_last_error() gives the message.
 *     No C++ exception crosses this boundary.
 *   - tensors are caller-owned DEVICE buffers (fp32, contiguous, reference layout [B][C][L]); the library
 *     never frees them and only owns its weights / workspace / graphs.
 *   - `stream` is a hipStream_t passed as void* (e.g. torch.cuda.current_stream().cuda_stream); all work
 *     is enqueued there, nothing synchronises the device except adf_load_weight's final packing, which is
 *     also stream-ordered.
 *   - one handle is not thread-safe; distinct handles are independent.
 *   - a handle belongs to the device that was current at adf_create: every entry point makes that device current for
 *     its duration (and restores the caller's), so pointers and the stream must belong to that device.
 *   - memory the library keeps grows only up to a cap: at most 4 (B, L) workspaces per handle and 8 captured sampler
 *     graphs per workspace are retained (least recently used ones are released).
 */
#ifndef AUDIODIFFUSER_AMD_H
#define AUDIODIFFUSER_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct of this header grows or an entry point's argument list changes; a binding compares it with
 * adf_abi_version() of the library it loaded before the first call (audiodiffuser_amd/_lib.py does; INTEGRATION.md's C example too).
 * 3: adf_sampler_run(n_injected), adf_sampler_desc.reflow, adf_get_counters.
 * 4: ADF_FLAG_NEAREST_UPSAMPLE (adf_net_config.flags bit 1; state-dict keys ...upsample.2.weight / .bias), WaveNetNoise in bf16 at 64 / 128
 *    residual channels, adf_debug_tap on a WaveNet handle keeps every layer while all of them fit 512 MiB (256 MiB before).
 * 5: ADF_DTYPE_F32X3 (a third value of adf_net_config.dtype: fp32 storage, every GEMM operand split into bf16 hi + lo, three bf16 MFMAs per product).
 * 6: adf_unet2d_config / adf_unet2d_create (the Imagen-style UNet2dBase, exact fp32).
 * 7: adf_set_preconditioning (ADF_PRECOND_EDM / VE / VP / V_EDM) and adf_debug_coef_rows.  The preconditioning kind travels as handle state, in the
 *    style of adf_set_dynamic_threshold: adf_sampler_desc and the argument list of adf_denoise are unchanged, so a caller that fills only the
 *    fields of version 6 and never calls the setter still gets EluDiffusion's rows.
 *    Added without a bump (new symbols only, nothing of the above changes): adf_istft_config and the four adf_istft_* entry points;
 *    the four adf_stft_* entry points (WaveToSpec), which take the same adf_istft_config; adf_debug_tap_stats, adf_debug_up_tile_plan and adf_debug_rb_block_plan.
 *    Also without a bump (new values of existing int arguments / fields; no struct grows and no argument list changes, and a library of version 7 without
 *    them refuses both with its "unknown kind" errors): ADF_PRECOND_RF / ADF_PRECOND_RF_EDM (ReFlow) and ADF_SAMPLER_RF_EULER (ReflowEulerSampler).
 *    Added without a bump (new symbols only): adf_diffusion_loss with the three ADF_LOSS_* kinds, and adf_loss_calls -- a counter of its own,
 *    because adf_run_counters must not grow within a version.
 *    Added without a bump (new symbols only): adf_sampler_run_table and adf_sampler_table_nfe with their own adf_table_desc / adf_table_step /
 *    adf_table_eval and the three ADF_CLIP_* modes (VESampler, VPSampler, VSampler, VEulerSampler).  No ADF_SAMPLER_* or ADF_PRECOND_* kind is added:
 *    adf_sampler_desc, its kinds and adf_set_preconditioning are as they were.
 *    Added without a bump (new symbols only): adf_sampler_run_program and adf_sampler_program_nfe with adf_prog_desc / adf_prog_op and the ADF_PROG_*
 *    constants (VDPMSampler, VUniPCSampler).  adf_table_eval is reused as it is.  The table and the program are two public forms of one
 *    loop: the library lowers both to one internal op list and one driver runs it; neither form's structs, messages or cache keys depend on that.
 *    Added without a bump (new symbols only): adf_dit_config and adf_dit_create (DiT); everything after create is the existing surface.
 *    Added without a bump (new symbols only): adf_dac_config, adf_dac_create, adf_dac_forward and adf_dac_output_length (the DAC decoder and the
 *    decode half of FineTuneAutoencoder).  Such a handle has its own forward entry; the denoiser and sampler calls refuse it.
 *    Added without a bump (a new symbol and a new value of an existing field): adf_dac_encode and ADF_DAC_KIND_ENCODER (the DAC encoder and the
 *    encode half of FineTuneAutoencoder), on the unchanged adf_dac_config layout. */
#define ADF_ABI_VERSION 7
int adf_abi_version(void);

#define ADF_MAX_LAYERS 12

#define ADF_DTYPE_F32 0  /* parity mode: fp32 storage, exact-fp32 MFMA */
#define ADF_DTYPE_BF16 1 /* throughput mode: bf16 storage, fp32 accumulate */
#define ADF_DTYPE_F32X3 2 /* split-bf16 mode (UNet1dBase, the ADM UNetModel and DiT): fp32 storage as ADF_DTYPE_F32; a GEMM operand x is staged as bf16 hi = rn(x) and
                             lo = rn(x - hi) (x = hi + lo to 2^-17) and a product is hi*hi + hi*lo + lo*hi on the bf16 MFMA with fp32 accumulation:
                             ~1e-5 relative per layer against the exact-fp32 mode, inside the 1e-3 bar of the reference comparison, at the bf16 MFMA rate / 3 */

/* Hyper-parameters of UNet1dBase; same meaning as the reference kwargs. */
typedef struct adf_net_config {
    int32_t channels, num_filters, window_length, stride, in_channels, out_channels;
    int32_t resnet_groups, kernel_multiplier_downsample;
    int32_t num_layers;                     /* len(multipliers) - 1 */
    int32_t multipliers[ADF_MAX_LAYERS + 1];
    int32_t factors[ADF_MAX_LAYERS];
    int32_t num_blocks[ADF_MAX_LAYERS];
    int32_t attentions[ADF_MAX_LAYERS];
    int32_t attention_heads, attention_multiplier;
    int32_t use_skip_scale, use_attention_bottleneck;
    int32_t dtype;                          /* ADF_DTYPE_* */
    int32_t flags;                          /* ADF_FLAG_* */
    int32_t num_classes;                    /* > 0: class_cond=True with that many labels (LabelEmbedder); 0: unconditional */
} adf_net_config;

#define ADF_FLAG_SEPARATE_GN_STATS 1 /* compute GroupNorm statistics in a separate pass instead of the GEMM epilogue */
#define ADF_FLAG_NEAREST_UPSAMPLE 2  /* UNet1dBase(use_nearest_upsample=True): Upsample1d = nearest x f -> ReflectionPad1d(1) -> Conv1d(k = 3)
                                        (unet1d.py:236-246; state-dict keys ...upsample.2.weight / .bias); every factor >= 2 */

#define ADF_SAMPLER_EDM 0       /* EDMSampler: Heun + optional churn      */
#define ADF_SAMPLER_EDM_ALPHA 1 /* EDMAlphaSampler: generalised RK2        */
#define ADF_SAMPLER_DPM_MULTISTEP 2 /* DPMSampler(multisteps=True, x0_pred=True, log_time_spacing=False) */
#define ADF_SAMPLER_DPM2 3      /* DPM2Sampler ("DPM2 Karras", optional churn)   sampler_edm.py:401-493 */
#define ADF_SAMPLER_ADPM2 4     /* ADPM2Sampler ("DPM2 a Karras", ancestral)     stochastic_sampler_edm.py:35-100 */
#define ADF_SAMPLER_LMS 5       /* LMSSampler ("LMS Karras"), order 1..4         sampler_edm.py:1134-1190 */
#define ADF_SAMPLER_DPM2M 7     /* DPM2MSampler ("DPM-Solver++(2M) Karras"); needs num_steps + 1 sigmas   sampler_edm.py:1056-1131;
                                   with `reflow` the class of the same name in stochastic_sampler_edm.py:180-259 */
#define ADF_SAMPLER_UNIPC 8     /* UniPCSampler (variant bh2), order 1..3, x0 or noise prediction, both spacings   sampler_edm.py:807-1053 */
#define ADF_SAMPLER_DPM_SINGLESTEP 6 /* DPMSampler(multisteps=False, x0_pred=True) sampler_edm.py:568-622, :769-805 */
#define ADF_SAMPLER_ADPMPP2S 9  /* ADPMPP2SSampler ("DPM++ 2S a Karras", ancestral; one draw per step with sigma_next > 0)   stochastic_sampler_edm.py:102-178 */
#define ADF_SAMPLER_RF_EULER 10 /* ReflowEulerSampler (rectified flow: Euler, or Heun where sigma_next != 0); the denoiser output is the velocity (ADF_PRECOND_RF);
                                   needs num_steps + 1 sigmas; reads only num_steps, use_heun, use_graph; final clamp   sampler_rf.py:7-70 */

typedef struct adf_sampler_desc {
    int32_t kind;
    int32_t num_steps;   /* the reference constructor's num_steps */
    float s_tmin, s_tmax, s_churn, s_noise;  /* EDM */
    int32_t use_heun;    /* EDM, EDM_ALPHA, RF_EULER */
    float alpha;         /* EDM_ALPHA */
    int32_t order;       /* DPM, UniPC: 1..3; LMS: 1..4 */
    float sigma_data;    /* EluDiffusion.sigma_data */
    int32_t use_graph;   /* capture the whole step loop into one hipGraph and replay it */
    float rho, eta;      /* ADPM2 */
    int32_t log_time_spacing;  /* DPM (both kinds), UniPC: the reference's log_time_spacing flag (sampler_edm.py:518, :546-556, :824) */
    int32_t eps_pred;          /* DPM (both kinds), UniPC: 1 = the reference's x0_pred=False (noise prediction, :700-706, :841-846) */
    int32_t reflow;            /* DPM2M: 1 = read the denoiser output as a velocity, denoised = x - output * sigma (stochastic_sampler_edm.py:214-215) */
} adf_sampler_desc;

/* Hyper-parameters of WaveNetNoise (wavenet.py:154-157) and of the ResidualGroup it builds (:120: dim_in 128, dim_mid 512,
 * dim_out 512; ResidualBlock's Linear(512, C) fixes dim_out = 512 in the reference). */
typedef struct adf_wavenet_config {
    int32_t residual_channels, residual_layers, dilation_cycle;
    int32_t dim_in, dim_mid, dim_out;
    int32_t dtype;                          /* ADF_DTYPE_*; BF16 (MFMA kernels) needs residual_channels = 64, 128 or 256 */
} adf_wavenet_config;

/* Hyper-parameters of the ADM-style UNetModel (unet2d_oai.py:410-430).  attention_ds holds the downsample factors at which
 * attention runs -- what the constructor derives from `attention_resolutions` and `image_size` (:433-436). */
#define ADF_ADM_MAX_LEVELS 8
typedef struct adf_adm_config {
    int32_t in_channels, model_channels, out_channels, num_res_blocks;
    int32_t n_mult; int32_t channel_mult[ADF_ADM_MAX_LEVELS];
    int32_t n_attention_ds; int32_t attention_ds[ADF_ADM_MAX_LEVELS];
    int32_t conv_resample, num_heads, num_head_channels, use_scale_shift_norm, resblock_updown, use_new_attention_order;
    int32_t num_classes;                    /* 0 = unconditional; > 0: LabelEmbedder + adf_set_condition (labels, guidance), as for adf_create */
    int32_t dtype;                          /* ADF_DTYPE_F32, _BF16 or _F32X3 */
} adf_adm_config;

/* Hyper-parameters of the Imagen-style UNet2dBase (unet2d.py:623-667) in the layout the device runs: memory_efficient, cross-embed initial conv,
 * global-context gates, pixel-shuffle upsampling, no text / condition encoder.  init_kernel_sizes: the cross-embed kernel sizes sorted ascending
 * (all odd); layer_cross_attns only decides which resnet blocks carry a (never run) cross_attn module in the state dict. */
#define ADF_U2D_MAX_LEVELS 8
#define ADF_U2D_MAX_INIT_KERNELS 4
typedef struct adf_unet2d_config {
    double ff_mult;
    int32_t dim, cond_dim, channels, channels_out, num_classes;
    int32_t n_levels; int32_t dim_mults[ADF_U2D_MAX_LEVELS];
    int32_t layer_attns[ADF_U2D_MAX_LEVELS]; int32_t layer_cross_attns[ADF_U2D_MAX_LEVELS];
    int32_t num_resnet_blocks, resnet_groups, attn_heads;
    int32_t layer_attns_depth, layer_mid_attns_depth, attend_at_middle;
    int32_t n_init_kernels; int32_t init_kernel_sizes[ADF_U2D_MAX_INIT_KERNELS];
    int32_t learned_sinu_pos_emb_dim, num_time_tokens;
    int32_t scale_skip_connection, final_resnet_block;
    int32_t dtype;                          /* ADF_DTYPE_F32 only */
} adf_unet2d_config;

/* Hyper-parameters of DiT, the adaLN-Zero diffusion transformer (dit.py:282-300), as the device runs it: label or no conditioning, the plain
 * attention branch (no text context, no RoPE, no qk-l2norm).  mlp_hidden = int(hidden_size * mlp_ratio), what Mlp is built with (dit.py:238). */
typedef struct adf_dit_config {
    int32_t input_h, input_w;               /* input_size: the only (H, W) the net takes (PatchEmbed's strict_img_size); [B][C][L] inputs are H = 1 */
    int32_t patch_h, patch_w;               /* patch_size: divides input_size; patch_h * patch_w * in_channels in [4, 256] */
    int32_t in_channels;                    /* = out_channels */
    int32_t hidden_size;                    /* a multiple of 64, at most 1024 */
    int32_t depth, num_heads;               /* hidden_size / num_heads = 32 or 64 */
    int32_t mlp_hidden;                     /* a multiple of 32, at most 4096 */
    int32_t num_classes;                    /* 0 = unconditional; > 0: y_embedder (LabelEmbedder) + adf_set_condition (labels, guidance) */
    int32_t dtype;                          /* ADF_DTYPE_F32 or ADF_DTYPE_F32X3 */
} adf_dit_config;

typedef struct adf_handle adf_handle;

int adf_create(const adf_net_config* cfg, adf_handle** out);
/* A UNetModel (ADM) handle: x / out of adf_net_forward, adf_denoise, adf_sampler_run are [B][C][H][W] fp32 with L = H * W, the
 * shape given by adf_set_image_shape before the call.  On the device: scale-shift or additive conditioning, conv / pooled resampling, resblock up/down, either
 * attention order, unconditional (BASELINE config 4) or class-conditional.  Debug taps: "input_blocks.<i>", "middle_block",
 * "output_blocks.<i>" (the outputs of the reference's blocks).
 * dtype: ADF_DTYPE_F32 and ADF_DTYPE_F32X3 need model_channels to be a multiple of 32, ADF_DTYPE_BF16 of 64 (at most 256).  In the split-bf16 mode the
 * 3x3 / 1x1 convs and the attention at head dim 32 take bf16 hi + lo operands; the first and last conv, the GroupNorm kernels, pooling, nearest
 * upsampling and the embedding projections are the fp32 ones. */
int adf_adm_create(const adf_adm_config* cfg, adf_handle** out);
/* A UNet2dBase handle: the same 2-D conventions as a UNetModel handle (adf_set_image_shape first; H and W multiples of 2^n_levels).
 * forward(x, time = c_noise), optionally class-conditional (adf_set_condition).  Debug taps: "init_conv", "init_resnet_block", "downs.<i>",
 * "mid_block", "ups.<i>", "final_res_block" (the module outputs the reference's fixtures hold) and every stored intermediate. */
int adf_unet2d_create(const adf_unet2d_config* cfg, adf_handle** out);
/* A DiT handle (added without a version bump: new symbols only): the same 2-D conventions (adf_set_image_shape first, with exactly input_size; a
 * [B][C][L] input is H = 1, W = L).  forward(x, t = c_noise), optionally class-conditional (adf_set_condition; the label embedding joins the time
 * embedding before every adaLN modulation).  State-dict keys: pos_embed, x_embedder.proj.*, t_embedder.mlp.{0,2}.*, y_embedder.* (num_classes > 0),
 * blocks.<i>.attn.{to_q,to_kv,to_context,to_out}.weight (to_context is loaded and never read), blocks.<i>.mlp.{fc1,fc2}.*,
 * blocks.<i>.adaLN_modulation.1.*, final_layer.{linear,adaLN_modulation.1}.*.  ADF_DTYPE_F32: exact fp32, every Linear on v_mfma_f32_32x32x2_f32.
 * ADF_DTYPE_F32X3 (additive, no version bump; the same widths): the q|k|v projection, to_out, fc1 and fc2 of every block and its attention (Q K^T and
 * P V, key-tiled, any token count) take bf16 hi + lo operands, three bf16 MFMAs per product; the modulation GEMM, final_layer.linear and everything
 * that is not a GEMM stay the fp32 kernels.  The fp32 weight buffers stay the load target; the hi / lo planes are rebuilt before the first pass after
 * a load.  Route switches read from the environment at create (default 1): ADF_DIT_X3_LINEAR=0 keeps the fp32 token linear, ADF_DIT_X3_ATT=0 the fp32
 * vector attention in an ADF_DTYPE_F32X3 handle (both 0: bit for bit the ADF_DTYPE_F32 handle).  ADF_DTYPE_BF16 is refused.  The last kernel
 * has all three epilogues (raw, clamped, unclipped), so every preconditioning kind is one pass.  Debug taps ([B][D][T] as adf_debug_tap_copy lays
 * them out): "x_embedder", "c" ([B][D][1]), "blocks.<i>", "blocks.<i>.attn" / "blocks.<i>.mlp" (the branches before their gates), "final_layer"
 * (before unpatchify); the per-block taps exist while 3 * depth * B * T * D floats fit 512 MiB (beyond that, or with the route switch ADF_DIT_TAPS=0 in the
 * environment at create, the residual stream is updated in place and they are not kept). */
int adf_dit_create(const adf_dit_config* cfg, adf_handle** out);

/* The DAC decoder stack (added without a version bump: new symbols only), exact fp32: what turns a sampled latent into a waveform.
 *   ADF_DAC_KIND_DECODER      dac.py::Decoder(input_channel, channels, rates, d_out = 1) (src/models/backbones/dac/dac.py:108-137): a k = 7 conv, one
 *                             DecoderBlock per rate s (Snake, ConvTranspose1d of kernel 2 s, stride s, padding ceil(s / 2), three ResidualUnits with
 *                             dilations 1 / 3 / 9), Snake, a k = 7 conv to one channel, tanh.  Every stage width channels / 2**i must be a multiple of 32,
 *                             1 to 6 rates in [2, 16] (odd ones included).  A rate s maps a length L to (L - 1) s - 2 ceil(s / 2) + 2 s.
 *   ADF_DAC_KIND_AUTOENCODER  FineTuneAutoencoder.decode (src/models/backbones/dac_vae.py:37-71) with conv_kernel = 3: input_channel is latent_dim,
 *                             widths is intermediate_embedding_size (widths[0] = 1024, every entry a multiple of 32); channels and rates are
 *                             not read.  adf_dac_forward (decode) reads neither btnk_layer.* nor encoder_layers.*.
 *                             With adf_dac_encode the handle also serves FineTuneAutoencoder.encode(x, is_train=False): encoder_layers.* (Snake, k = 3
 *                             conv per width) and btnk_layer (a plain 1x1 conv to 2 latent_dim channels) are folded like the rest; d_out =
 *                             ADF_DAC_BTNK_TANH is tanh_btnk=True (any other value: False).
 *   ADF_DAC_KIND_ENCODER      dac.py::Encoder(d_model, strides, d_latent) (dac.py:57-84): input_channel = 1, channels = d_model, rates = strides,
 *                             d_out = d_latent.  A k = 7 conv from the waveform, one EncoderBlock per stride s (three ResidualUnits with dilations
 *                             1 / 3 / 9, Snake, Conv1d of kernel 2 s, stride s, padding ceil(s / 2) that doubles the width), Snake, a k = 3 conv to
 *                             d_latent.  d_model a multiple of 32 with d_model * 2**n_rates <= 8192, d_latent a multiple of 32 in [32, 8192], 1 to 6
 *                             strides in [2, 16].  A stride s maps a length L to floor((L + 2 ceil(s / 2) - 2 s) / s) + 1 (L / s for even s,
 *                             (L + 1) / s for odd s) and needs L >= 2 s - 2 ceil(s / 2); adf_dac_forward refuses a shorter L by name.
 * input_channel (decoder, autoencoder): a multiple of 4 in [4, 2048].  State-dict keys are the reference's, with the weight-norm pair of every conv (<conv>.bias,
 * <conv>.weight_g, <conv>.weight_v; weight_g of a ConvTranspose1d is [C_in][1][1]) and <snake>.alpha [1][C][1]; the folded weight
 * g v / ||v|| is rebuilt before the first pass after any (re)load.  Snake is x + sin^2(alpha x) / (alpha + 1e-9), fused into the staging of the conv
 * behind it.  Such a handle is no denoiser: adf_net_forward, adf_denoise, adf_diffusion_loss and the sampler calls refuse it with a message;
 * adf_dac_forward is its compute call, and the weight, tap and adf_device_bytes calls serve it as they serve every handle.
 * Debug taps (decoder): "model.0", "model.<i>" (every DecoderBlock), "model.<i>.block.1" (the transposed conv), "model.<i>.block.{2,3,4}" (the
 * ResidualUnits), "model.<n_rates + 2>" (the value before tanh, [B][1][L_out]); the per-unit taps exist while they fit 512 MiB (beyond that, or with the
 * route switch ADF_DAC_TAPS=0 in the environment at create, a unit adds into its input in place and only "model.0" and "model.<i>" are kept).
 * Autoencoder: "decoder_layers.<2 i>" (every conv); after adf_dac_encode "encoder_layers.<2 i + 1>" (every conv) and "btnk_layer" (the raw
 * [B][2 latent_dim][T] before chunk, clamp and tanh).  Encoder: "block.0", "block.<i>" (every EncoderBlock), "block.<i>.block.{0,1,2}" (the
 * ResidualUnits, under the same 512 MiB / ADF_DAC_TAPS rule), "block.<n_rates + 2>" (the result). */
#define ADF_DAC_KIND_DECODER 0
#define ADF_DAC_KIND_AUTOENCODER 1
#define ADF_DAC_KIND_ENCODER 2
#define ADF_DAC_BTNK_TANH 2                 /* adf_dac_config::d_out of an autoencoder built with tanh_btnk=True */
#define ADF_DAC_MAX_RATES 6
#define ADF_DAC_MAX_WIDTHS 8
typedef struct adf_dac_config {
    int32_t kind;                           /* ADF_DAC_KIND_* */
    int32_t input_channel;                  /* Decoder: input_channel; autoencoder: latent_dim; encoder: 1 */
    int32_t channels;                       /* Decoder: width behind the first conv; encoder: d_model */
    int32_t n_rates;
    int32_t rates[ADF_DAC_MAX_RATES];
    int32_t d_out;                          /* Decoder: 1; encoder: d_latent; autoencoder: ADF_DAC_BTNK_TANH or anything else */
    int32_t n_widths;
    int32_t widths[ADF_DAC_MAX_WIDTHS];     /* autoencoder: intermediate_embedding_size */
    int32_t dtype;                          /* ADF_DTYPE_F32 */
} adf_dac_config;
int adf_dac_create(const adf_dac_config* cfg, adf_handle** out);
/* in: fp32 [B][input_channel][T] on the handle's device; out: fp32 [B][1][adf_dac_output_length(h, T)] (decoder), [B][1024][T] (autoencoder) or
 * [B][d_latent][adf_dac_output_length(h, T)] (encoder: in is the waveform [B][1][T]).
 * Enqueued on `stream`; allocates only when (B, T) is new to the handle, so a later call with the same shape can be captured in a graph. */
int adf_dac_forward(adf_handle* h, const float* in, int B, int T, float* out, void* stream);
int64_t adf_dac_output_length(const adf_handle* h, int T);     /* -1: not a DAC handle, T < 1, or (encoder) T too short for a stage */
/* FineTuneAutoencoder.encode(x, is_train=False) on an ADF_DAC_KIND_AUTOENCODER handle (any other handle is refused with a message): in fp32
 * [B][1024][T]; mean_out fp32 [B][latent_dim][T] (tanh of it under ADF_DAC_BTNK_TANH); kl_out one fp32 on the device:
 * 0.5 mean_b sum_{c, t} (mean^2 + exp(logvar) - logvar - 1) with logvar clamped to [-30, 20], summed in a fixed order (bit-reproducible, no atomics).
 * Enqueued on `stream`; allocates only when (B, T) is new to encode on this handle.  adf_dac_forward (decode) on the same handle is unaffected. */
int adf_dac_encode(adf_handle* h, const float* in, int B, int T, float* mean_out, float* kl_out, void* stream);
int adf_set_image_shape(adf_handle* h, int H, int W);

/* Clipping of every denoiser evaluation from here on (adf_denoise, adf_sampler_run): 0 = clamp to [-1, 1] (the default), q in (0, 1] = the dynamic
 * thresholding of EluDiffusion(dynamic_threshold = q) -- per sample, scale = max(1, quantile(|x|, q)) (torch.quantile's linear interpolation),
 * x = clamp(x, -scale, scale) / scale.  Replaces src/models/components/utils.py:19-33 (`clip`) as called from diffusion.py:61. */
int adf_set_dynamic_threshold(adf_handle* h, float quantile);

/* Preconditioning of every denoiser evaluation from here on (adf_denoise, adf_sampler_run): which formulas turn a sigma into the row
 * (c_in, c_noise, c_skip, c_out) of out = clip(c_skip * x + c_out * net(c_in * x, c_noise)).  All in fp32 in the reference's order of operations
 * (src/models/components/diffusion.py):
 *   ADF_PRECOND_EDM    EluDiffusion  :232-241  ((s^2 + sd^2)^-1/2, ln(s) / 4, sd^2 / (s^2 + sd^2), s sd (s^2 + sd^2)^-1/2); sd = the sigma_data argument of
 *                                              adf_denoise / adf_sampler_desc (the default of a new handle)
 *   ADF_PRECOND_VE     VEDiffusion   :107-116  (1, ln(s / 2), 1, s)
 *   ADF_PRECOND_VP     VPDiffusion   :156-170  ((s^2 + 1)^-1/2, (M - 1) t(s), 1, -s), t(s) = (sqrt(beta_min^2 + 2 beta_d ln(1 + s^2)) - beta_min) / beta_d
 *   ADF_PRECOND_V_EDM  VDiffusion(for_edm=True) :296-326  (a, -2 ln s, a^2, -sqrt(sigmoid(2 ln s))), a = sqrt(sigmoid(-2 ln s)).  The estimate is returned
 *                                              UNCLIPPED, as in the reference: neither the clamp nor the dynamic threshold applies.
 *   ADF_PRECOND_RF     ReFlow(for_edm=False)    :388-418  (1, s, 0, 1): the "sigma" is the rectified-flow time t in [0, 1] and the result is the network's
 *                                              velocity itself (under guidance: the guided velocity), UNCLIPPED.  What ADF_SAMPLER_RF_EULER and
 *                                              ADF_SAMPLER_DPM2M with `reflow` drive.
 *   ADF_PRECOND_RF_EDM ReFlow(for_edm=True)     :379-418  (1 - t, t, 1 - t, -t), t = s / (s + 1): x0 = (1 - t) x - t v, UNCLIPPED, for the EDM-family samplers
 *                                              on RFEDMSchedule (sigma = t / (1 - t)).
 * beta_min, beta_d, M are read for ADF_PRECOND_VP only (doubles: beta_min^2, 2 beta_d and M - 1 are formed in double and then rounded to fp32, as torch
 * rounds the reference's Python scalars); sigma_data is ignored by every kind but ADF_PRECOND_EDM. */
#define ADF_PRECOND_EDM 0
#define ADF_PRECOND_VE 1
#define ADF_PRECOND_VP 2
#define ADF_PRECOND_V_EDM 3
#define ADF_PRECOND_RF 4
#define ADF_PRECOND_RF_EDM 5
int adf_set_preconditioning(adf_handle* h, int kind, double beta_min, double beta_d, double M);
/* A WaveNetNoise handle.  x / out of adf_net_forward, adf_denoise, adf_sampler_run are [B][1][T] (the reference's forward takes
 * audio [B][T] and returns [B][1][T]: same memory); any T >= 1.  Debug taps: "y<n>" = input of residual layer n including its
 * diffusion-step addend (kept while all of them fit 512 MiB), "skip" = the normalised skip sum. */
int adf_wavenet_create(const adf_wavenet_config* cfg, adf_handle** out);
void adf_destroy(adf_handle* h);
const char* adf_last_error(const adf_handle* h);   /* h may be NULL: error of the last failed adf_create */

/* state_dict interface: names/shapes are exactly the reference UNet1dBase.state_dict() keys */
int adf_num_weights(const adf_handle* h);
const char* adf_weight_name(const adf_handle* h, int index);
int64_t adf_weight_numel(const adf_handle* h, int index);
int adf_load_weight(adf_handle* h, const char* name, const float* dev_fp32, int64_t numel, void* stream);
int adf_weights_missing(const adf_handle* h);      /* number of tensors not loaded yet */

/* Class conditioning / classifier-free guidance for the calls that follow with the same B
 * (UNet1dBase.forward(classes=, cond_drop_prob=) unet1d.py:864-893, LabelEmbedder conditioner.py:59-111, the CFG branch
 * of Diffusion.denoise_fn diffusion.py:49-54).  classes_dev: int64 [B] labels on the device, or NULL to clear the
 * condition.  null_labels != 0: every sample uses the null embedding (cond_drop_prob = 1).  cond_scale applies to
 * adf_denoise / adf_sampler_run only: != 1 runs the network twice per evaluation (labels, null) and combines
 * null + (cond - null) * cond_scale before the EDM preconditioning.  A class-conditional network needs a condition. */
int adf_set_condition(adf_handle* h, const int64_t* classes_dev, int B, int null_labels, float cond_scale, void* stream);

/* out = net(x, t):  x [B][in_channels][L], t [B], out [B][out_channels][L] */
int adf_net_forward(adf_handle* h, const float* x, const float* t, float* out, int B, int L, void* stream);

/* out = clamp(c_skip*x + c_out*net(c_in*x, c_noise), -1, 1); sigmas_dev [B] or NULL (then `sigma` for all).  The rows and the clipping are those of
 * adf_set_preconditioning / adf_set_dynamic_threshold (defaults: EluDiffusion with `sigma_data`, clamp). */
int adf_denoise(adf_handle* h, const float* x_noisy, const float* sigmas_dev, float sigma, float sigma_data,
                float* out, int B, int L, void* stream);

/* The validation loss: Diffusion.forward / VPDiffusion.forward / ReFlow.forward under torch.no_grad() (src/models/components/diffusion.py:65-97,
 * :185-218, :420-442; called from diffunet_complex_module.py:116-125) as one call.  x, noise: [B][C][L] fp32, contiguous, 4-byte aligned;
 * sigmas_dev: [B] on the device (sigmas for the x0 kinds -- VPDiffusion's already mapped from t -- and times t for ADF_LOSS_RF); losses: [B] fp32.
 * Enqueues, in order:
 *   mix      x_noisy = fl(x + fl(s_b noise)) (x0 kinds) or fl(fl(fl(1 - t_b) x) + fl(t_b noise)) (RF): every operation rounded to fp32 on its own, so
 *            bit-equal to the reference's tensor expressions evaluated in fp32
 *   denoise  exactly what adf_denoise(h, x_noisy, sigmas_dev, 0, sigma_data, pred, B, L, stream) enqueues, with the handle's preconditioning, clipping and
 *            condition / guidance state (for ADF_LOSS_RF the handle is expected to be set to ADF_PRECOND_RF: pred is the raw velocity)
 *   loss     losses[b] = w(s_b) / N * sum_i fl(d_i d_i), N = C * L; d = fl(pred - x) with w = (s^2 + sd^2) / (s sd)^2 (ADF_LOSS_X0_EDM) or 1 / s^2
 *            (ADF_LOSS_X0_INV_SIGMA2); d = fl(fl(noise - x) - pred) with w = 1 (ADF_LOSS_RF).  Summed in double in a fixed order (no atomics: the same
 *            bits on every run and every device), w / N formed in double from the fp32 sigma, one rounding to fp32.
 * x_noisy_out / pred_out may each be NULL; if given they receive the noisy input and the denoiser output of this call ([B][C][L]; an output that
 * overlaps x, noise or the other output is refused).  The handle needs in_channels == out_channels; a 2-D handle needs adf_set_image_shape first, a class-conditional one adf_set_condition.
 * Refuses (adf_last_error names the argument) a null x, noise, sigmas_dev or losses, an unknown kind, sigma_data <= 0 for ADF_LOSS_X0_EDM.
 * adf_run_counters is left as it is, every field (neither denoise_calls nor net_passes counts the loss's evaluation); adf_loss_calls counts the successful calls and is how a caller tells that the device path ran.
 * The first loss call on a (B, L) workspace allocates; after it the call neither allocates nor synchronises and can be captured into the caller's graph
 * (which then holds addresses of that workspace: replay it only while its (B, L) is among the 4 workspaces the handle keeps). */
#define ADF_LOSS_X0_EDM        0   /* EluDiffusion  diffusion.py:65-97, :243-245 */
#define ADF_LOSS_X0_INV_SIGMA2 1   /* VEDiffusion :118-120, VPDiffusion :152-154 (sigmas already mapped from t, :185-218) */
#define ADF_LOSS_RF            2   /* ReFlow(for_edm=False) :420-442 */
int adf_diffusion_loss(adf_handle* h, int kind, const float* x, const float* noise, const float* sigmas_dev, float sigma_data,
                       float* losses, float* x_noisy_out, float* pred_out, int B, int L, void* stream);
int64_t adf_loss_calls(const adf_handle* h);   /* successful adf_diffusion_loss calls */

/* Full sampling loop.  sigmas_host: the schedule tensor (host, n_sigmas entries) the reference passes as
 * `sigmas`; noise: unit-variance [B][C][L]; injected_noise: [n_injected][B][C][L] draws replacing
 * randn_like, one per step in the reference's order (required when the EDM / DPM2 sampler churns and always for
 * ADPM2, which adds noise every step; may be NULL otherwise).  n_injected = number of [B][C][L] draws behind the
 * pointer: fewer than the sampler consumes (num_steps for EDM, num_steps - 1 for DPM2 / ADPM2) is an error. */
int adf_sampler_run(adf_handle* h, const adf_sampler_desc* desc, const float* sigmas_host, int n_sigmas,
                    const float* noise, const float* injected_noise, int n_injected, float* out, int B, int L, void* stream);
int adf_sampler_nfe(const adf_sampler_desc* desc, const float* sigmas_host, int n_sigmas);

/* The table form of the op loop: a sampler whose every branch and scalar depends on the schedule and the constructor arguments only, handed over as one
 * host record per step.  What runs VESampler / VPSampler (src/models/components/sampler_edm.py:31-227) and VSampler / VEulerSampler
 * (sampler_vobj.py:31-194); audiodiffuser_amd/samplers.py builds their tables.  With x the fp32 state, eps the record's draw and D a denoiser
 * evaluation out = clip(c_skip x_in + c_out net(c_in x_in, c_noise)), step i is
 *     x_hat = a0 x + a1 eps
 *     D1    = denoise(eval1, x_hat)
 *     x_e   = b0 x_hat + b1 D1 + b2 eps                     (second == 0: x = x_e, the step ends here)
 *     D2    = denoise(eval2, x_e)
 *     x     = c0 x_hat + c1 D1 + c2 x_e + c3 D2
 * and the run is x = x0_scale * noise, the steps, then clamp(-1, 1) where final_clamp != 0.  Every linear combination is one fused pass over the state,
 * in place; an operand whose coefficient is zero is not read (so a record with a1 == b2 == 0 needs no draw, and a0 == 1, a1 == 0 launches nothing).
 * The rows are taken as given -- the handle's preconditioning kind is not consulted -- and land in the per-run table adf_debug_coef_rows returns; the
 * time embedding and the FiLM projections of all evaluations are computed once at the head of the run, as in adf_sampler_run.  `clip` of an evaluation:
 *     ADF_CLIP_NONE        the estimate as it is
 *     ADF_CLIP_CONFIGURED  what the handle is set to: clamp(-1, 1), the dynamic threshold of adf_set_dynamic_threshold, or nothing under an unclipped
 *                          preconditioning kind (ADF_PRECOND_V_EDM, _RF, _RF_EDM)
 *     ADF_CLIP_UNIT        clamp(-1, 1) whatever the handle is set to
 * Class labels and guidance (adf_set_condition) apply as in adf_sampler_run: cond_scale != 1 is two passes per evaluation.  injected_noise:
 * [n_injected][B][C][L]; a record that reads eps reads draw number `draw` of it.  use_graph: the whole run is captured once as a single chain and
 * replayed; the cache key holds the descriptor and table bytes and the handle's condition, clipping and preconditioning state.  adf_run_counters moves
 * as for adf_sampler_run (sampler_runs + 1, sampler_evals + the table's NFE, graph_replays + 1 when replayed).
 * Refused before anything is launched, with a message that starts with "adf_sampler_run_table: " and names the argument: a null desc, steps, noise
 * or out; num_steps <= 0; a non-finite x0_scale, coefficient or row entry; an unknown clip; second != 0 with b0 == b1 == b2 == 0 (D2 without x_e);
 * a record that reads eps with injected_noise null or draw outside [0, n_injected).
 * adf_sampler_table_nfe: host only; the evaluations of the table (one per record, two where second != 0), or -1 for a table the run would refuse
 * for what the table itself holds (the draws are not known here). */
#define ADF_CLIP_NONE 0
#define ADF_CLIP_CONFIGURED 1
#define ADF_CLIP_UNIT 2
typedef struct adf_table_eval {
    float c_in, c_noise, c_skip, c_out;
    int32_t clip;                 /* ADF_CLIP_* */
} adf_table_eval;
typedef struct adf_table_step {
    float a0, a1;
    adf_table_eval eval1;
    float b0, b1, b2;
    int32_t second;               /* != 0: the step has the second evaluation and the c0..c3 update */
    adf_table_eval eval2;         /* read where second != 0 */
    float c0, c1, c2, c3;         /* read where second != 0 */
    int32_t draw;                 /* index of the [B][C][L] draw this record's eps is; read where a1 != 0 or b2 != 0 */
} adf_table_step;
typedef struct adf_table_desc {
    int32_t num_steps;            /* records behind `steps` */
    float x0_scale;               /* x = x0_scale * noise */
    int32_t final_clamp;
    int32_t use_graph;
} adf_table_desc;
int adf_sampler_run_table(adf_handle* h, const adf_table_desc* desc, const adf_table_step* steps, const float* noise, const float* injected_noise,
                          int n_injected, float* out, int B, int L, void* stream);
int adf_sampler_table_nfe(const adf_table_desc* desc, const adf_table_step* steps);

/* The program form of the op loop: a sampler with memory (a linear multistep method) whose every branch and scalar depends on the schedule and the constructor
 * arguments only, handed over as a straight-line host program over ADF_PROG_SLOTS state buffers (fp32 [B][C][L] each).  What runs
 * sampler_vobj.DPMSampler and sampler_vobj.UniPCSampler (src/models/components/sampler_vobj.py:196-732); audiodiffuser_amd/samplers.py builds their
 * programs.  Slot 0 starts as x0_scale * noise, every other slot as unwritten.  An op is
 *     ADF_PROG_EVAL   slot[dst] = clip(c_skip x + c_out net(c_in x, c_noise)), x = slot[src]; `eval` is an adf_table_eval, read as in the table form
 *     ADF_PROG_LIN    slot[dst] = sum_{j < n_terms} coef[j] * slot[slot[j]], 1 <= n_terms <= ADF_PROG_TERMS, clamped to [-1, 1] where clamp != 0;
 *                     one fused pass; dst may be one of the operands
 * and the sample is slot[result_slot] after the last op.  There are no draws.  A method's history (its earlier model outputs) stays where it was
 * written: the host renames slots from step to step, nothing is copied.  No evaluation, guided or not, uses a slot as scratch.
 * In everything else the run behaves as adf_sampler_run_table: labels and guidance from adf_set_condition, the rows taken as given and every c_noise
 * embedded once at the head of the run (adf_debug_coef_rows returns them), use_graph captures the run once and replays it, with the cache key holding
 * the descriptor and program bytes and the handle's condition, clipping and preconditioning state; adf_run_counters moves by sampler_runs + 1,
 * sampler_evals + the number of EVAL ops, graph_replays + 1 when replayed.
 * Refused before anything is launched, with a message that starts with "adf_sampler_run_program: " and names the argument: a null desc, ops, noise or
 * out; num_ops <= 0; a non-finite x0_scale; an unknown kind; dst, src, slot[j] or result_slot outside [0, ADF_PROG_SLOTS); a read (src, slot[j],
 * result_slot) of a slot that neither the start state nor an earlier op has written; an EVAL with dst == src; n_terms outside 1 .. ADF_PROG_TERMS;
 * the same slot twice in one LIN; a non-finite coef[j] or row entry; an unknown clip; a program without an EVAL.
 * adf_sampler_program_nfe: host only; the EVAL ops of the program, or -1 for a program the run would refuse for what it holds. */
#define ADF_PROG_EVAL 0
#define ADF_PROG_LIN 1
#define ADF_PROG_SLOTS 8
#define ADF_PROG_TERMS 5
typedef struct adf_prog_op {
    int32_t kind;                 /* ADF_PROG_* */
    int32_t dst;
    int32_t src;                  /* EVAL: the slot evaluated */
    adf_table_eval eval;          /* EVAL */
    int32_t n_terms;              /* LIN */
    int32_t slot[ADF_PROG_TERMS]; /* LIN */
    float coef[ADF_PROG_TERMS];   /* LIN */
    int32_t clamp;                /* LIN */
} adf_prog_op;
typedef struct adf_prog_desc {
    int32_t num_ops;              /* ops behind `ops` */
    int32_t result_slot;
    float x0_scale;               /* slot 0 = x0_scale * noise */
    int32_t use_graph;
} adf_prog_desc;
int adf_sampler_run_program(adf_handle* h, const adf_prog_desc* desc, const adf_prog_op* ops, const float* noise, float* out, int B, int L, void* stream);
int adf_sampler_program_nfe(const adf_prog_desc* desc, const adf_prog_op* ops);

/* Parity-test support: copy an internal activation of the LAST adf_net_forward/adf_denoise call, converted to
 * fp32 [B][C][L].  Names follow oracle/unet1d.py taps ("to_in", "down0.conv", "down0.block1", "mid.attn", ...).  "class_emb" (not among
 * adf_debug_tap_name's): the [B][cdim][1] label embedding of the last adf_set_condition, while a condition is set.  "cfg.cond" / "cfg.null"
 * (likewise): the two raw network outputs [B][out_channels][L] of the last evaluation, where it ran under guidance (cond_scale != 1). */
int adf_debug_tap_shape(adf_handle* h, const char* name, int* C, int* L);
int adf_debug_tap_copy(adf_handle* h, const char* name, float* out_fp32, void* stream);
/* The GroupNorm statistics that the launch which stored tap `name` reduced with it: [B][groups][2] doubles (sum, sum of squares per sample and
 * group) copied to out_host (host memory; may be null to ask only for *groups).  An error if that tensor was stored without statistics. */
int adf_debug_tap_stats(adf_handle* h, const char* name, double* out_host, int* groups, void* stream);
/* Host arithmetic only (no device is touched): the tile plan of the transposed-conv kernel (csrc/adf_gemm_up.h) for B samples of L input rows of
 * one of its four shapes (cin -> cout, factor f): rows per tile, work items (sample x tile x column pass), rounds of 256 workgroups, and the
 * rows of a sample's last tile past L.  Returns nonzero for any other shape. */
int adf_debug_up_tile_plan(int cin, int cout, int f, int B, int L, int* tile_rows, int* items, int* rounds, int* dead_rows);
/* Host arithmetic only: the K-block table the resblock conv kernel's raw form (csrc/adf_gemm_rb.h, bf16) gets for B samples of L rows and n columns.
 * phase_c = 0: Conv1d(K, stride f) over C channels folded to 3 taps over f C channels (L = output rows); phase_c > 0: the 3-tap form of a transposed
 * conv over C channels with n / phase_c phases (K, f unused).  min_tiles: fewest workgroup tiles the route takes; zskip: the ADF_RB_ZSKIP switch.
 * Out: rows per tile, 128-column halves per tile, three-tap and two-tap K blocks per tile, and whether the launch takes the phase form.  Returns
 * nonzero for a shape the kernel does not take. */
int adf_debug_rb_block_plan(int K, int f, int C, int phase_c, int n, int B, int L, int min_tiles, int zskip, int* tile_rows, int* nh, int* nb3, int* nb2,
                            int* phase2);
/* The dynamic threshold alone, in place on x_dev [B][per_sample] (tests: exactness of the order statistics against torch.quantile). */
int adf_debug_dyn_threshold(adf_handle* h, float* x_dev, int B, long long per_sample, float quantile, void* stream);
/* The (c_in, c_noise, c_skip, c_out) rows of the last adf_sampler_run on this handle, one per denoiser evaluation in order: copies
 * min(max_rows, rows) * 4 floats to out_dev (device) and returns the number of rows of that run through *n_rows.  After an adf_denoise call
 * at the same shape: the rows of that call instead (one for a scalar sigma, B for per-sample sigmas). */
int adf_debug_coef_rows(adf_handle* h, float* out_dev, int max_rows, int* n_rows, void* stream);
int adf_debug_tap_count(adf_handle* h);
const char* adf_debug_tap_name(adf_handle* h, int index);

/* What the handle has enqueued so far.  The plugin classes fall back to a host-side loop of tensor ops around a foreign `fn`
 * / `net` (interface compatibility); these counters are how a caller -- and every GPU sampler test -- tells that the device loop
 * of adf_sampler_run ran instead.  net_passes counts network passes enqueued by host code: a captured loop counts once at
 * capture, its replays are graph_replays (sampler_evals adds the evaluations of every run, replayed or not). */
typedef struct adf_run_counters {
    int64_t sampler_runs;     /* successful adf_sampler_run calls */
    int64_t sampler_evals;    /* denoiser evaluations those runs performed on the device */
    int64_t graph_captures;   /* step loops captured into a hipGraph */
    int64_t graph_replays;    /* adf_sampler_run calls served by hipGraphLaunch */
    int64_t denoise_calls;    /* adf_denoise calls */
    int64_t net_passes;       /* network passes enqueued by host code (eager, warm-up, capture) */
} adf_run_counters;
int adf_get_counters(const adf_handle* h, adf_run_counters* out);

/* Bytes of device memory held by the handle (weights + workspaces). */
int64_t adf_device_bytes(const adf_handle* h);

/* Instrumentation for bench.py: the two GEMM launches of resblock `level` of the last forward are replayed `iters` times
 * with HIP events on `stream`, exactly as the network pass issues them (GroupNorm table from the input statistics,
 * output statistics in the epilogue), each iteration on another copy of the operands (>= 3 copies, >= 320 MiB in
 * rotation) so that the 256 MiB Infinity Cache cannot serve them.  *_block1 = conv1, *_block2 = conv2 (+ residual). */
int adf_bench_resblock(adf_handle* h, int B, int L, int level, int iters, float* ms_block1, float* ms_block2,
                       double* algo_bytes_block1, double* algo_bytes_block2, double* flops_block1,
                       double* flops_block2, void* stream);
/* One of the two launches only (conv = 1 | 2); *copies = number of operand copies in rotation = number of untimed warm-up
 * launches that precede the `iters` timed ones (lets a profiler pass pick out the timed dispatches). */
int adf_bench_layer(adf_handle* h, int B, int L, int level, int conv, int iters, float* ms, double* algo_bytes, double* flops,
                    int* copies, void* stream);

/* WaveNetNoise handles: residual layer `layer` of the last pass replayed `iters` times (after 2 untimed launches) with HIP events
 * on `stream`.  The working set of one launch at bench sizes (y, y_next, fp32 skip sum: > 5 GB at B = 128, T = 22050) is far beyond
 * the 256 MiB Infinity Cache, so no operand rotation is needed. */
int adf_bench_wavenet_layer(adf_handle* h, int B, int T, int layer, int iters, float* ms, double* algo_bytes, double* flops, void* stream);

/* The two memory-bound kernels of adf_diffusion_loss alone (any handle; its network is not run): the mix and the per-block squared-error sums over
 * B rows of N fp32 elements in buffers of their own, `iters` launches each after 2 untimed ones, with HIP events on `stream`.  rf != 0: the ADF_LOSS_RF
 * forms (the error pass then reads the noise too).  *bytes_* = the tensor traffic of one launch.  Allocates and frees 16 B N bytes per call. */
int adf_bench_loss_kernels(adf_handle* h, int rf, int B, long long N, int iters, float* ms_mix, float* ms_partial, double* bytes_mix,
                           double* bytes_partial, void* stream);

/* SpecToWave: the tail of DiffUnetComplexModule.synthesize_from_noise (src/models/diffunet_complex_module.py:90-99) in one launch --
 * view_as_complex(permute(spec)) + spec_back (src/models/utils.py:22-28) + torch.istft(window, normalized, center=True, length=None).
 * spec is the sampler's output as it leaves adf_sampler_run: fp32 [B][2][n_fft / 2 + 1][T], channel 0 real, 1 imaginary.  audio is fp32
 * [B][audio_len] with audio_len = hop_length * (T - 1), 16-byte aligned.  The inverse DFT, the window and the overlap-add are one exact-fp32
 * MFMA GEMM against a windowed cosine / sine basis built in double on the host.
 *   n_fft even in [32, 1024]; hop_length a multiple of 32 in [32, 256]; ceil(n_fft / hop_length) <= 8; center must be 1; T >= 2;
 *   spec_abs_exponent > 0, spec_factor > 0.  window: n_fft floats on the HOST, or NULL for the periodic Hann window; the sum of its shifted
 *   squares must stay above 1e-11 over the kept samples (torch.istft's NOLA check).
 * A plan belongs to the device current at adf_istft_create; adf_istft_run makes it current, enqueues on `stream`, and neither allocates nor
 * synchronises.  Every function returns 0 on success; adf_last_error(NULL) gives the message of the last failure. */
typedef struct adf_istft_config {
    int32_t n_fft, hop_length, center, normalized;
    double spec_abs_exponent, spec_factor;
} adf_istft_config;
typedef struct adf_istft_plan adf_istft_plan;
int adf_istft_create(const adf_istft_config* cfg, const float* window, adf_istft_plan** out);
/* Host only (touches no device): the tables the plan is built from, with D = ceil(n_fft / hop_length), F = n_fft / 2 + 1, s = sqrt(n_fft) / n_fft when
 * normalized, else 1 / n_fft, a_0 = a_{F-1} = 1 and every other a_k = 2:
 *   basis [2][D * hop_length][F]:  basis[0][m][k] = w[m] a_k cos(2 pi m k / n_fft) s,  basis[1][m][k] = -w[m] a_k sin(2 pi m k / n_fft) s, with
 *                                  basis[1][m][0] = basis[1][m][F-1] = 0 and rows m >= n_fft zero; computed in double, rounded once
 *   wsq   [D * hop_length]:        w[m]^2, zero for m >= n_fft
 * Either output may be NULL (both NULL: the arguments are checked and nothing is written). */
int adf_istft_basis(const adf_istft_config* cfg, const float* window, float* basis, float* wsq);
int adf_istft_run(adf_istft_plan* plan, const float* spec, int B, int T, float* audio, int64_t audio_len, void* stream);
void adf_istft_destroy(adf_istft_plan* plan);

/* WaveToSpec: the head of DiffUnetComplexModule.forward (src/models/diffunet_complex_module.py:109-115) in one launch --
 * torch.stft(window, normalized, center=True, pad_mode="reflect", return_complex=True) + spec_fwd (src/models/utils.py:8-19) + cat(real, imag).
 * audio is fp32 [B][L], rows back to back and only 4-byte aligned (any L > n_fft / 2: torch refuses a shorter row for the reflect padding, so does
 * adf_stft_run); spec is fp32 [B][2][n_fft / 2 + 1][T] with T = 1 + L / hop_length, channel 0 real, 1 imaginary -- the tensor the networks and
 * adf_istft_run take.  Samples no frame reaches are ignored.  The padding is never materialised; the windowed DFT is one exact-fp32 MFMA GEMM against
 * a cosine / sine basis built in double on the host, and spec_fwd runs on its accumulators.  A bin whose magnitude is exactly 0 gives 0.
 *   The accepted arguments are those of adf_istft_*: n_fft even in [32, 1024]; hop_length a multiple of 32 in [32, 256];
 *   ceil(n_fft / hop_length) <= 8; center must be 1; spec_abs_exponent > 0, spec_factor > 0.  window: n_fft floats on the HOST, or NULL for the
 *   periodic Hann window; there is no overlap-add condition in this direction, but a window that is zero everywhere (or not finite) is refused.
 *   adf_stft_run refuses L <= n_fft / 2, L >= 2^30, T != 1 + L / hop_length and B outside [1, 65535].
 * Arguments are checked before any device is looked for.  A plan belongs to the device current at adf_stft_create; adf_stft_run makes it current,
 * enqueues on `stream`, and neither allocates nor synchronises.  Every function returns 0 on success; adf_last_error(NULL) gives the message of the
 * last failure, which starts with the function's name and names the argument. */
typedef struct adf_stft_plan adf_stft_plan;
int adf_stft_create(const adf_istft_config* cfg, const float* window, adf_stft_plan** out);
/* Host only (touches no device): the table the plan is built from, with F = n_fft / 2 + 1 and s = n_fft^-1/2 when normalized, else 1:
 *   basis [2][F][n_fft]:  basis[0][k][m] = w[m] cos(2 pi m k / n_fft) s,  basis[1][k][m] = -w[m] sin(2 pi m k / n_fft) s, with the rows
 *                         basis[1][0] and basis[1][F-1] exactly zero; computed in double, rounded once
 * basis may be NULL (the arguments are checked and nothing is written).  adf_istft_basis has a second table (the squared window of its overlap-add
 * envelope); nothing in this direction needs one, so there is no second output here. */
int adf_stft_basis(const adf_istft_config* cfg, const float* window, float* basis);
int adf_stft_run(adf_stft_plan* plan, const float* audio, int B, int64_t L, float* spec, int T, void* stream);
void adf_stft_destroy(adf_stft_plan* plan);

#ifdef __cplusplus
}
#endif
#endif

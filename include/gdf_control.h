/* gdf_control.h — the ControlNet as a native model of libgdf.so.
 *
 * What it replaces in the reference (paths relative to /root/reference/feature): the call
 *   `controlnet(latent_model_input, t, encoder_hidden_states=prompt_embeds, controlnet_cond=image, conditioning_scale=1, guess_mode=False,
 *    added_cond_kwargs=..., return_dict=False)`                                         components/controlnet.py:95-130
 * i.e. diffusers' ControlNetModel.forward (0.32.2; the class is not vendored in the reference tree, the wiring is restated from the published
 * source): the UNet's time / add embeddings, `conv_in(sample) + controlnet_cond_embedding(cond)`, the UNet's down blocks and mid block, and
 * one 1x1 convolution per skip tensor and for the mid block's output.
 *
 * The output is ONE device block in the layout gdf_forward_res reads (gdf.h: gdf_residual_bytes / gdf_residual_info): the producer writes the
 * block through the function the consumer reads it with.  Conventions as in gdf.h.
 */
#ifndef GDF_CONTROL_H
#define GDF_CONTROL_H
#include "gdf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A ControlNetModel over the encoder half of `arch` (the UNet's descriptor: out_channels and the up path are not used).
 *   cond_channels            conditioning_embedding_out_channels; (16, 32, 96, 256) is the only supported value (csrc/cond_embed.hip)
 *   conditioning_channels    channels of the control image, 1..8 (3)
 * Parameters in diffusers' state_dict naming: conv_in.*, time_embedding.*, add_embedding.* (text_time), down_blocks.*, mid_block.* as in the
 * UNet; controlnet_cond_embedding.conv_in / blocks.0..5 / conv_out .weight (OIHW) and .bias; controlnet_down_blocks.k.weight (C, C, 1, 1) and
 * .bias for every skip k in the order of gdf_residual_info; controlnet_mid_block.weight / .bias.  The gdf_model_* functions of gdf.h work on
 * the model unchanged; it has no hooks (gdf_model_hook_count is 0). */
int gdf_controlnet_create(const gdf_arch_desc* arch, const int cond_channels[4], int conditioning_channels, gdf_model** out);

/* The same model as a parameter table alone — names, shapes, count, in the order gdf_controlnet_create registers them — without touching a device
 * (a loader can check a checkpoint against it on any host).  gdf_model_param_count / _name / _shape and gdf_model_destroy apply; setting a
 * parameter or creating a plan on it is an error. */
int gdf_controlnet_layout(const gdf_arch_desc* arch, const int cond_channels[4], int conditioning_channels, gdf_model** out);

/* The static op program for (batch, latent size): the UNet's down and mid program op for op, the conditioning embedding in front of it and
 * one dense GEMM behind every skip.  opts: stream_fp32, reserved[0] (shared ctx), reserved[1] (split operand classes) and reserved[2] (CUs)
 * mean what they mean for gdf_plan_create; the conditioning embedding always runs plain fp16 (an 8-bit image is exact in fp16).  The plan has
 * no hooks and no early exit.  gdf_plan_workspace_bytes, gdf_plan_set_graph, gdf_plan_graph_stats, gdf_plan_num_ops, gdf_plan_op_kernel,
 * gdf_plan_set_timing and gdf_plan_destroy apply. */
int gdf_controlnet_plan_create(gdf_model* m, int batch, int lat_h, int lat_w, int n_ctx, const gdf_plan_opts* opts, gdf_plan** out);

/* One ControlNet forward.  latents, timesteps, ctx, add_text_embeds, add_time_ids: exactly gdf_forward's (the reference hands the
 * ControlNet the UNet's inputs).  cond_image: (B, conditioning_channels, 8 lat_h, 8 lat_w) NCHW in [0, 1], cond_dtype GDF_F16 or GDF_F32.
 * residual_block_out: 256-byte aligned, gdf_controlnet_residual_bytes bytes; tensor i is written at the offset gdf_residual_info reports, fp16
 * channels-last (B, H, W, C); bytes between tensors are not touched.  conditioning_scale is 1 and guess_mode off.
 * A UNet plan handed to this entry, and a ControlNet plan handed to gdf_forward / gdf_forward_res, are refused with an error. */
int gdf_controlnet_forward(gdf_plan* p, const void* latents, const float* timesteps, const void* ctx, const void* add_text_embeds,
                           const float* add_time_ids, const void* cond_image, int cond_dtype, void* residual_block_out, void* workspace,
                           void* stream);
/* bytes of the block a ControlNet plan writes (== gdf_residual_bytes of its architecture, batch and latent size); 0 for any other plan */
size_t gdf_controlnet_residual_bytes(const gdf_plan* p);

#ifdef __cplusplus
}
#endif
#endif /* GDF_CONTROL_H */

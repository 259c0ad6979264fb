"""ctypes binding of liblatte_amd.so — the ONLY compute backend of this package.

There is no CPU / PyTorch fallback: if the HIP library is missing or no MI355X is visible the
product path raises.  `import torch` must precede loading the library so that it binds to the HIP
runtime torch already loaded (one runtime per process -> torch data_ptr()s and streams are valid).
"""
import ctypes
import os

import torch  # noqa: F401  (must be imported before the engine library, see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblatte_amd.so")

c_int, c_i64, c_f32, c_void, c_char = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_char_p
c_u64 = ctypes.c_uint64


class LatteError(RuntimeError):
    pass


class ModelConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("input_size", "patch_size", "in_channels", "hidden_size", "depth", "num_heads",
                                     "mlp_hidden", "num_frames", "num_classes", "learn_sigma", "extras",
                                     "compute_dtype")]


class T2VConfig(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("num_attention_heads", "attention_head_dim", "in_channels", "out_channels", "num_layers",
                                     "sample_size", "patch_size", "cross_attention_dim", "caption_channels", "video_length",
                                     "max_text_tokens", "compute_dtype")]


class T5Config(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("d_model", "d_kv", "num_heads", "d_ff", "num_layers", "vocab_size",
                                     "relative_attention_num_buckets", "relative_attention_max_distance")] \
        + [("layer_norm_epsilon", c_f32), ("compute_dtype", c_int)]


class VideoPlan(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("kind", "src_h", "src_w", "out_h", "out_w", "mid_h", "mid_w", "crop_i", "crop_j",
                                     "reg_y", "reg_x", "reg_h", "reg_w")] + [("scale_h", c_f32), ("scale_w", c_f32)]


T2V_PLAN_COLS = 12   # LATTE_T2V_PLAN_COLS of include/latte_amd.h (= LATTE_PLAN_COLS)
PLAN_COLS = 12       # LATTE_PLAN_COLS
DTYPES = {"bf16": 0, "bfloat16": 0, "f16": 1, "fp16": 1, "float16": 1}

# name -> (restype, argtypes); mirrors include/latte_amd.h and include/latte_amd_debug.h
PROTOTYPES = {
    "latte_last_error": (c_char, []),
    "latte_version": (c_char, []),
    "latte_schedule_create": (c_int, [c_int, c_char, c_char, ctypes.POINTER(c_void)]),
    "latte_schedule_destroy": (None, [c_void]),
    "latte_schedule_set_model_types": (c_int, [c_void, c_int, c_int, c_int]),
    "latte_schedule_num_timesteps": (c_int, [c_void]),
    "latte_schedule_timestep_map": (c_int, [c_void, c_void, c_int]),
    "latte_schedule_table": (c_int, [c_void, c_char, c_void, c_int]),
    "latte_engine_create": (c_int, [ctypes.POINTER(ModelConfig), c_int, ctypes.POINTER(c_void)]),
    "latte_engine_destroy": (None, [c_void]),
    "latte_engine_set_option": (c_int, [c_void, c_char, c_i64]),
    "latte_engine_get_option": (c_int, [c_void, c_char, ctypes.POINTER(c_i64)]),
    "latte_engine_load_tensor": (c_int, [c_void, c_char, c_void, c_i64, c_int, c_void]),
    "latte_engine_check_weights": (c_int, [c_void]),
    "latte_engine_num_keys": (c_int, [c_void]),
    "latte_engine_key": (c_char, [c_void, c_int]),
    "latte_engine_temb_table": (c_int, [c_void, c_void, c_void, c_void]),
    "latte_engine_set_temb_table": (c_int, [c_void, c_void, c_void, c_void]),
    "latte_engine_set_text_embedding": (c_int, [c_void, c_void, c_int, c_void]),
    "latte_forward": (c_int, [c_void, c_void, c_void, c_void, c_int, c_void, c_void]),
    "latte_forward_with_cfg": (c_int, [c_void, c_void, c_void, c_void, c_int, c_f32, c_void, c_void]),
    "latte_sampler_step_ex": (c_int, [c_void, c_int, c_int, c_f32, c_int, c_void, c_void, c_void, c_void, c_void, c_int, c_int,
                                      c_int, c_int, c_int, c_void, c_void, c_void]),
    "latte_sampler_step": (c_int, [c_void, c_int, c_int, c_f32, c_int, c_void, c_void, c_void, c_int, c_int, c_int,
                                   c_int, c_void, c_void, c_void]),
    "latte_sample_loop": (c_int, [c_void, c_void, c_int, c_f32, c_int, c_f32, c_void, c_void, c_int, c_int, c_int,
                                  c_void, c_void, c_void, c_void]),
    "latte_sample_loop_ex": (c_int, [c_void, c_void, c_int, c_f32, c_int, c_int, c_f32, c_void, c_void, c_int, c_int, c_int,
                                     c_void, c_void, c_void, c_void]),
    "latte_invert_loop": (c_int, [c_void, c_void, c_int, c_int, c_f32, c_void, c_void, c_int, c_int, c_int, c_void, c_void, c_void]),
    "latte_sample_loop_known": (c_int, [c_void, c_void, c_int, c_f32, c_int, c_int, c_f32, c_void, c_void, c_int, c_int, c_int,
                                        c_void, c_void, c_int, c_int, c_void, c_void, c_void, c_void]),
    "latte_known_chain_slabs": (c_int, [c_void, c_int, c_f32, c_int, c_int, c_int, c_int, ctypes.POINTER(c_i64)]),
    "latte_known_blend": (c_int, [c_void, c_void, c_void, c_void, c_u64, c_u64, c_f32, c_f32, c_int, c_int, c_int, c_int, c_int,
                                  c_void]),
    "latte_sample_plan_loop": (c_int, [c_void, c_int, c_f32, c_void, c_void, c_int, c_int, c_void, c_void, c_void, c_void]),
    "latte_window_plan": (c_int, [c_int, c_int, c_int, c_void, c_void, c_int]),
    "latte_window_gather": (c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_window_merge": (c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_sample_loop_windows": (c_int, [c_void, c_void, c_int, c_f32, c_int, c_int, c_f32, c_void, c_void, c_int, c_int, c_int,
                                          c_void, c_void, c_void, c_int, c_int, c_void]),
    "latte_sample_plan_loop_windows": (c_int, [c_void, c_int, c_f32, c_void, c_void, c_int, c_int, c_void, c_void, c_void, c_int, c_int,
                                               c_void]),
    "latte_q_sample": (c_int, [c_void, c_void, c_void, c_void, c_int, c_i64, c_void, c_void]),
    "latte_training_workspace_floats": (c_i64, [c_int, c_i64]),
    "latte_training_losses": (c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_void,
                                      c_i64, c_void, c_void, c_void, c_void]),
    "latte_prior_bpd": (c_int, [c_void, c_void, c_int, c_i64, c_void, c_void]),
    "latte_bpd_workspace_floats": (c_i64, [c_int, c_i64]),
    "latte_bpd_terms": (c_int, [c_void, c_int, c_int, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_void, c_i64,
                                c_void, c_void, c_void, c_i64, c_void, c_void]),
    "latte_bpd_loop": (c_int, [c_void, c_void, c_int, c_void, c_void, c_int, c_int, c_int, c_void, c_void, c_void, c_void, c_void]),
    "latte_trainer_create": (c_int, [ctypes.POINTER(ModelConfig), c_int, ctypes.POINTER(c_void)]),
    "latte_trainer_destroy": (None, [c_void]),
    "latte_trainer_num_params": (c_int, [c_void]),
    "latte_trainer_param_key": (c_char, [c_void, c_int]),
    "latte_trainer_param_offset": (c_i64, [c_void, c_int]),
    "latte_trainer_param_numel": (c_i64, [c_void, c_int]),
    "latte_trainer_total_numel": (c_i64, [c_void]),
    "latte_trainer_bind": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void]),
    "latte_trainer_set_frozen": (c_int, [c_void, c_void, c_void, c_int, c_void]),
    "latte_trainer_sync_weights": (c_int, [c_void, c_void]),
    "latte_trainer_forward_backward": (c_int, [c_void, c_void, c_int, c_void, c_void, c_void, c_void, c_int, c_void, c_void, c_void]),
    "latte_trainer_begin": (c_int, [c_void, c_void, c_int, c_void, c_void, c_void, c_void, c_int, c_void, c_void, c_void]),
    "latte_trainer_create_joint": (c_int, [ctypes.POINTER(ModelConfig), c_int, c_int, ctypes.POINTER(c_void)]),
    "latte_trainer_forward_backward_joint": (c_int, [c_void, c_void, c_int, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_void, c_void,
                                                     c_void]),
    "latte_trainer_begin_joint": (c_int, [c_void, c_void, c_int, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_void, c_void, c_void]),
    "latte_trainer_num_stages": (c_int, [c_void]),
    "latte_trainer_stage_range": (c_int, [c_void, c_int, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]),
    "latte_trainer_backward_stage": (c_int, [c_void, c_int, c_void]),
    "latte_trainer_forward": (c_int, [c_void, c_void, c_void, c_void, c_int, c_void, c_void]),
    "latte_trainer_seed": (c_int, [c_void, c_void, c_void]),
    "latte_trainer_input_grad": (c_int, [c_void, c_void, c_void]),
    "latte_trainer_optimizer_step": (c_int, [c_void, c_f32, c_f32, c_f32, c_f32, c_f32, c_int, c_f32, c_int, c_f32, c_void, c_void]),
    "latte_trainer_set_option": (c_int, [c_void, c_char, ctypes.c_double]),
    "latte_trainer_lora_enable": (c_int, [c_void, c_int, c_f32, c_int]),
    "latte_trainer_lora_num_params": (c_int, [c_void]),
    "latte_trainer_lora_param_key": (c_char, [c_void, c_int]),
    "latte_trainer_lora_param_offset": (c_i64, [c_void, c_int]),
    "latte_trainer_lora_param_numel": (c_i64, [c_void, c_int]),
    "latte_trainer_lora_total_numel": (c_i64, [c_void]),
    "latte_trainer_bind_lora": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    "latte_trainer_lora_merge": (c_int, [c_void, c_void, c_void, c_void]),
    "latte_trainer_scaler_state": (c_int, [c_void, ctypes.POINTER(ctypes.c_double)]),
    "latte_trainer_set_scaler_state": (c_int, [c_void, ctypes.POINTER(ctypes.c_double)]),
    "latte_profile_forward": (c_int, [c_void, c_void, c_void, c_void, c_int, c_void, c_void, c_void, c_int, c_void]),
    "latte_profile_forward_ex": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_void, c_void, c_void, c_int, c_void]),
    "latte_t2v_create": (c_int, [ctypes.POINTER(T2VConfig), c_int, ctypes.POINTER(c_void)]),
    "latte_t2v_destroy": (None, [c_void]),
    "latte_t2v_num_keys": (c_int, [c_void]),
    "latte_t2v_key": (c_char, [c_void, c_int]),
    "latte_t2v_load_tensor": (c_int, [c_void, c_char, c_void, c_i64, c_int, c_void]),
    "latte_t2v_check_weights": (c_int, [c_void]),
    "latte_t2v_set_option": (c_int, [c_void, c_char, c_i64]),
    "latte_t2v_forward": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_void, c_void]),
    "latte_t2v_set_text": (c_int, [c_void, c_void, c_void, c_int, c_int, c_void]),
    "latte_t2v_guided_ddim_loop": (c_int, [c_void, c_void, c_int, c_int, c_void, c_void, c_void, c_f32, c_int, c_void]),
    "latte_t2v_guided_ddim_loop_known": (c_int, [c_void, c_void, c_int, c_int, c_void, c_void, c_void, c_f32, c_void, c_void, c_void,
                                                 c_int, c_void]),
    "latte_t2v_guided_linear_loop": (c_int, [c_void, c_void, c_int, c_int, c_void, c_void, c_f32, c_int, c_void]),
    "latte_t2v_guided_ddim_loop_windows": (c_int, [c_void, c_void, c_int, c_int, c_void, c_void, c_void, c_f32, c_int, c_int, c_int,
                                                   c_void]),
    "latte_t2v_guided_linear_loop_windows": (c_int, [c_void, c_void, c_int, c_int, c_void, c_void, c_f32, c_int, c_int, c_int, c_void]),
    "latte_bench_gemm": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_f32), c_void]),
    "latte_vae_create": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_void)]),
    "latte_vae_create_temporal": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_void)]),
    "latte_vae_destroy": (None, [c_void]),
    "latte_vae_num_keys": (c_int, [c_void]),
    "latte_vae_key": (c_char, [c_void, c_int]),
    "latte_vae_load_tensor": (c_int, [c_void, c_char, c_void, c_i64, c_int, c_void]),
    "latte_vae_check_weights": (c_int, [c_void]),
    "latte_vae_decode": (c_int, [c_void, c_void, c_int, c_f32, c_int, c_void, c_void]),
    "latte_vae_profile_decode": (c_int, [c_void, c_void, c_int, c_f32, c_int, c_void, c_void, c_void, c_int, c_void]),
    "latte_vae_create_encoder": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_void)]),
    "latte_vae_encode": (c_int, [c_void, c_void, c_int, c_int, c_void, c_f32, c_int, c_void, c_void]),
    "latte_vae_posterior": (c_int, [c_void, c_void, c_int, c_int, c_f32, c_int, c_void, c_void]),
    "latte_moment_sample": (c_int, [c_void, c_int, c_i64, c_int, c_void, c_int, c_void, c_u64, c_u64, c_f32, c_int, c_void, c_void]),
    "latte_vae_profile_encode": (c_int, [c_void, c_void, c_int, c_int, c_void, c_f32, c_int, c_void, c_void, c_void, c_int, c_void]),
    "latte_video_transform_plan": (c_int, [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(VideoPlan)]),
    "latte_video_transform": (c_int, [c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_void, c_void, c_void]),
    "latte_t5_create": (c_int, [ctypes.POINTER(T5Config), c_int, c_int, ctypes.POINTER(c_void)]),
    "latte_t5_destroy": (None, [c_void]),
    "latte_t5_num_keys": (c_int, [c_void]),
    "latte_t5_key": (c_char, [c_void, c_int]),
    "latte_t5_load_weight": (c_int, [c_void, c_char, c_void, ctypes.POINTER(c_i64), c_int, c_void]),
    "latte_t5_check_weights": (c_int, [c_void]),
    "latte_t5_forward": (c_int, [c_void, c_void, c_void, c_int, c_int, c_void, c_void]),
    # test hooks
    "latte_debug_t5_embed": (c_int, [c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_t5_rmsnorm": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_f32, c_void]),
    "latte_debug_t5_bucket": (c_int, [c_int, c_int, c_int]),
    "latte_debug_t5_bias_table": (c_int, [c_void, c_int, c_int, c_int, c_int, c_void, c_void]),
    "latte_debug_t5_attention": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_t5_gated_act": (c_int, [c_void, c_void, c_void, c_int, c_int, c_void]),
    "latte_debug_t5_pack": (c_int, [c_void, c_void, c_void, c_i64, c_void]),
    "latte_debug_t5_proj_splits": (c_int, [c_int, c_int]),
    "latte_debug_t5_proj": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_gemm_lo8": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_int, c_void]),
    "latte_debug_attention_split8": (c_int, [c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_i64, c_i64, c_i64, c_int, c_void]),
    "latte_debug_pack_w4": (c_int, [c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_ln_modulate_split4": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_gemm_lo4": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int,
                                     c_int, c_int, c_void]),
    "latte_debug_pack_w8": (c_int, [c_void, c_void, c_i64, c_int, c_void]),
    "latte_debug_ln_modulate_split8": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_qkv_attention_split8": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                                 c_void]),
    "latte_debug_gemm": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int,
                                 c_int, c_int, c_void]),
    "latte_debug_gemm_gelu": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_gemm_choice": (c_int, [c_int, c_int, c_int, c_int]),
    "latte_debug_qkv_attention_fusable": (c_int, [c_int, c_int, c_int, c_int, c_int, c_i64]),
    "latte_debug_gemm_tn_plan": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "latte_debug_attention": (c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_i64, c_i64, c_i64, c_int,
                                      c_void]),
    "latte_debug_cross_attention": (c_int, [c_void, c_int, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_i64, c_i64,
                                            c_i64, c_int, c_void]),
    "latte_debug_small_linear": (c_int, [c_int, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int,
                                         c_void]),
    "latte_debug_patch_embed": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_final_layer": (c_int, [c_void, c_void, c_void, c_int, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_int, c_void]),
    "latte_debug_text_proj": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_gated_split_reduce": (c_int, [c_void, c_void, c_int, c_i64, c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_adaln_single": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_cond_rows": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_mask_bias": (c_int, [c_void, c_void, c_i64, c_void]),
    "latte_debug_plan_check": (c_int, [c_void, c_int, c_int, c_i64, c_int, c_int]),
    "latte_debug_t2v_linear_step": (c_int, [c_void] * 8 + [c_int] * 5 + [c_f32] * 10 + [c_int, c_void]),
    "latte_debug_linear_step": (c_int, [c_void] * 8 + [c_int] * 6 + [c_f32] * 10 + [c_int, c_void]),
    "latte_debug_qkv_attention": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                          c_int, c_void]),
    "latte_debug_qkv_attention_trace": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int,
                                                c_int, c_int, c_int, c_void]),
    "latte_debug_attention_bwd": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_i64, c_i64, c_i64,
                                          c_int, c_void]),
    "latte_debug_gemm_tn": (c_int, [c_void, c_void, c_void, c_void, c_i64, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_gemm_tn_colsum": (c_int, [c_void, c_void, c_void, c_void, c_void, c_i64, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_ln_modulate": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_void, c_int,
                                        c_int, c_int, c_void]),
    "latte_debug_convert": (c_int, [c_void, c_void, c_i64, c_int, c_void]),
    "latte_debug_gated_add_ln": (c_int, [c_void, c_void, c_void, c_int, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int,
                                         c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_ln_bwd": (c_int, [c_void, c_void, c_void, c_int, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_void,
                                   c_void, c_int, c_void, c_void, c_void, c_i64, c_int, c_void]),
    "latte_debug_gate_bwd": (c_int, [c_void, c_void, c_void, c_int, c_void, c_void, c_i64, c_void, c_int, c_int, c_int, c_int, c_int,
                                     c_int, c_void]),
    "latte_debug_split_reduce": (c_int, [c_void, c_int, c_i64, c_i64, c_void, c_int, c_void, c_void]),
    "latte_debug_colsum_half": (c_int, [c_void, c_int, c_int, c_void, c_i64, c_void, c_int, c_int, c_void, c_void]),
    "latte_debug_rows_sum": (c_int, [c_void, c_int, c_i64, c_int, c_void, c_int, c_void, c_void]),
    "latte_debug_naive_gemm": (c_int, [c_void, c_i64, c_i64, c_void, c_i64, c_i64, c_void, c_i64, c_i64, c_int, c_int, c_int, c_f32,
                                       c_int, c_int, c_void, c_i64, c_void, c_void]),
    "latte_debug_embedding_bwd": (c_int, [c_void, c_void, c_void, c_int, c_int, c_void, c_void]),
    "latte_debug_silu_bwd": (c_int, [c_void, c_void, c_void, c_i64, c_int, c_void]),
    "latte_debug_sumsq_blocks": (c_int, []),
    "latte_debug_grad_norm": (c_int, [c_void, c_i64, c_void, c_f32, c_int, c_void, c_void, c_void]),
    "latte_debug_adamw_ema": (c_int, [c_void, c_void, c_void, c_void, c_void, c_i64, c_f32, c_f32, c_f32, c_f32, c_f32, c_int, c_f32,
                                      c_void, c_void, c_void]),
    "latte_debug_gated_add": (c_int, [c_void, c_void, c_void, c_int, c_void, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_gelu": (c_int, [c_void, c_void, c_void, c_i64, c_int, c_int, c_void]),
    "latte_debug_tfreq": (c_int, [c_void, c_void, c_int, c_void]),
    "latte_debug_gather_i64": (c_int, [c_void, c_void, c_void, c_int, c_void]),
    "latte_debug_joint_split": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_i64, c_void]),
    "latte_debug_joint_merge": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_i64, c_void]),
    "latte_debug_unpatchify_bwd": (c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_im2col_patch": (c_int, [c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_add_rows": (c_int, [c_void, c_void, c_i64, c_void]),
    "latte_debug_scale_f32_dev": (c_int, [c_void, c_void, c_int, c_i64, c_void]),
    "latte_debug_silu_rows": (c_int, [c_void, c_void, c_i64, c_void]),
    "latte_debug_transpose_f32": (c_int, [c_void, c_void, c_int, c_int, c_void]),
    "latte_debug_widen": (c_int, [c_void, c_void, c_i64, c_int, c_void]),
    "latte_debug_stage_finalize": (c_int, [c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_void, c_int, c_void, c_void, c_void,
                                           c_int, c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_void]),
    "latte_debug_adaln_dc": (c_int, [c_void, c_int, c_int, c_void, c_i64, c_int, c_int, c_void, c_int, c_void, c_i64, c_void, c_void]),
    "latte_debug_narrow_outer": (c_int, [c_void, c_int, c_void, c_int, c_int, c_int, c_void, c_i64, c_i64, c_void, c_void, c_void, c_i64,
                                         c_int, c_void, c_int, c_void]),
    "latte_debug_narrow_dx": (c_int, [c_void, c_int, c_void, c_int, c_int, c_void, c_int, c_void]),
    "latte_debug_patch_embed_dgrad": (c_int, [c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void, c_void]),
    "latte_debug_pack_weights": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_void]),
    "latte_debug_pack_weight": (c_int, [c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_pack_weights_lora": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_f32,
                                              c_int, c_void]),
    "latte_debug_lora_table": (c_int, [ctypes.POINTER(ModelConfig), c_int, c_f32, c_int, c_int, c_void, c_int, ctypes.POINTER(c_i64),
                                       ctypes.POINTER(c_i64), ctypes.POINTER(c_int), ctypes.POINTER(c_i64)]),
    "latte_debug_lora_down": (c_int, [c_void, c_void, c_void, c_int, c_int, c_int, c_f32, c_int, c_void]),
    "latte_debug_lora_outer_plan": (c_int, [c_int, c_int, ctypes.POINTER(c_int)]),
    "latte_debug_lora_outer": (c_int, [c_void, c_void, c_void, c_void, c_i64, c_int, c_int, c_int, c_int, c_int, c_int, c_void, c_int,
                                       c_void]),
    "latte_debug_loss_grad": (c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_void,
                                      c_void]),
    "latte_debug_fill_normal": (c_int, [c_void, c_i64, c_u64, c_u64, c_void]),
    "latte_debug_tr16_probe": (c_int, [c_void, c_void]),
    "latte_debug_set_choice": (c_int, [c_char, c_int]),
    "latte_debug_dma_probe": (c_int, [c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_conv3x3": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_void]),
    "latte_debug_vae_trace": (c_int, [c_void, c_void, c_int, c_f32, c_int, c_void, c_void, c_void, c_void]),
    "latte_debug_vae_encode_trace": (c_int, [c_void, c_void, c_int, c_int, c_int, c_void, c_void, c_void, c_void]),
    "latte_debug_conv3x3_down_f32": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_vae_enc_conv_in": (c_int, [c_void, c_int, c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_vae_enc_tail": (c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_conv3rows_f32": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_conv3x3_f32": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void]),
    "latte_debug_groupnorm_f32": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_groupnorm": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_groupnorm_ex": (c_int, [c_void, c_int, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_f32, c_int, c_void,
                                         c_int, c_void]),
    "latte_debug_vae_post_quant": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_f32, c_void]),
    "latte_debug_vae_conv_in": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_vae_conv_out": (c_int, [c_void, c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_int, c_int, c_void]),
    "latte_debug_vae_softmax_rows": (c_int, [c_void, c_void, c_int, c_int, c_f32, c_void]),
    "latte_debug_vae_time_conv_out": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_int, c_void]),
    "latte_debug_vae_pack_conv_t": (c_int, [c_void, c_void, c_void, c_void, c_int, c_int, c_void]),
    "latte_debug_vae_scale_by_sigmoid": (c_int, [c_void, c_void, c_int, c_void, c_void]),
    "latte_debug_vae_pack_conv_w": (c_int, [c_void, c_void, c_void, c_int, c_int, c_void]),
    "latte_debug_convert_split": (c_int, [c_void, c_void, c_void, c_i64, c_void]),
}

_lib = None


def load_library():
    """Load liblatte_amd.so (raises LatteError when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("LATTE_AMD_LIB") or LIB_PATH     # LATTE_AMD_LIB: a compiler-flag A/B build (latte_amd/build.py: LATTE_BUILD_TAG), tools only
    if not os.path.exists(path):
        raise LatteError(
            f"{path} not found: build it with `python -m latte_amd.build` (hipcc, gfx950). "
            "latte_amd has no CPU or PyTorch fallback.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue  # reported by tests/test_abi.py; entry points of later build stages
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def require_gpu():
    if not torch.cuda.is_available():
        raise LatteError("latte_amd needs an MI355X (gfx950) visible to PyTorch-ROCm; there is no CPU fallback")


def check(rc):
    if rc != 0:
        msg = load_library().latte_last_error()
        raise LatteError((msg or b"unknown error").decode() + f" [code {rc}]")


def stream_ptr():
    return c_void(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return c_void(t.data_ptr()) if t is not None else c_void(None)


def to_device(args, kwargs, current, bf16_message):
    """The device a holder class's ``.to(*args, **kwargs)`` names: the str / torch.device among the arguments (a bare "cuda" gets the
    current index), else ``current``.  ``torch.bfloat16`` raises the caller's ``bf16_message``; other dtypes are accepted and ignored."""
    dev = current
    for a in list(args) + list(kwargs.values()):
        if isinstance(a, (str, torch.device)):
            dev = torch.device(a)
            if dev.type == "cuda" and dev.index is None:
                dev = torch.device("cuda", torch.cuda.current_device())
        elif a == torch.bfloat16:
            raise LatteError(bf16_message)
    return dev


def sync_weights(lib, family, handle, sd, device, optional=()):
    """Load every tensor the engine ``handle`` lists (``latte_<family>_key(i)``, family "engine" | "t2v" | "vae") from the state dict
    ``sd`` as fp32 on ``device``, check that nothing is missing, and wait for the packs.  Keys in ``optional`` may be absent."""
    num_keys, key, load_tensor, check_weights = (getattr(lib, f"latte_{family}_{n}")
                                                 for n in ("num_keys", "key", "load_tensor", "check_weights"))
    with torch.cuda.device(device):
        for i in range(num_keys(handle)):
            k = key(handle, i).decode()
            if k not in sd:
                if k in optional:
                    continue
                raise LatteError(f'Missing key(s) in state_dict: "{k}"')
            t = sd[k].detach().to(device=device, dtype=torch.float32).contiguous()
            check(load_tensor(handle, k.encode(), ptr(t), t.numel(), 1, stream_ptr()))
        check(check_weights(handle))
        torch.cuda.current_stream().synchronize()

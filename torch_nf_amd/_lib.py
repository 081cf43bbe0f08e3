"""ctypes binding of libtnf_hip.so (the C ABI declared in include/tnf.h).

This is the only place the package touches native code.  The library is built
in-tree by `__graft_entry__.build()` / `make -C torch_nf_amd/csrc`; if it is
missing the import fails loudly -- there is no CPU or PyTorch fallback for the
flow arithmetic anywhere in this package.
"""
import contextlib
import ctypes
import os

import torch  # imported first so the HIP runtime torch ships is the one the library binds to

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TNF_LIB_PATH") or os.path.join(_HERE, "lib", "libtnf_hip.so")  # override: kernel A/B builds

F32, F64 = 0, 1
LD_STORE, LD_ADD, LD_SUB = 0, 1, -1
FUSE_AUTO, FUSE_LAYER, FUSE_FLOW = 0, 1, 2
OPT_FORCE_GENERIC, OPT_FLOW_VARIANT, OPT_LAYER_VARIANT, OPT_COND_VARIANT, OPT_TRAIN_BWD_FP32 = 1, 2, 3, 4, 5
OPT_OPERAND_PREC = 6
OPT_REV_VARIANT = 7
EUNSUPPORTED = -2
DIAG_BWD_LAYER_FP32, DIAG_BWD_LAYER_F16, DIAG_BWD_GENERIC, DIAG_BWD_FLOW_REV = 0, 1, 2, 3
DIAG_MAF_BWD_MFMA, DIAG_MAF_BWD_GENERIC, DIAG_BWD_WIDE = 4, 5, 6
DIAG_FLOW_FUSED2, DIAG_FLOW_FUSED2_FWD, DIAG_FLOW_FUSED3, DIAG_FLOW_F16, DIAG_FLOW_FP32 = 7, 8, 9, 10, 11
DIAG_FLOW_RANGE2, DIAG_FLOW_RANGE2_FWD, DIAG_COUPLING_MFMA, DIAG_COND_FLOW = 12, 13, 14, 15
DIAG_FLOW_PADDED, DIAG_FLOW_PADDED_FWD, DIAG_COUPLING_WIDE = 16, 17, 18
DIAG_FAMILIES = 19
EF_MVN, EF_DIRICHLET = 0, 1
EF_COUNT_DOT, EF_COUNT_DOT_BWD = 0, 1  # tnf_ef_launch_count
MOG_COUNT_LOGPROB, MOG_COUNT_LOGPROB_BWD, MOG_COUNT_SAMPLE = 0, 1, 2  # tnf_mog_launch_count
ABC_COUNT_SMC, ABC_COUNT_PROPOSE, ABC_COUNT_NOISE = 0, 1, 2  # tnf_abc_launch_count
ABC_MAX_D, ABC_MAX_SMC_D, ABC_MAX_TRIALS = 21, 6, 1 << 24  # include/tnf_abc.h
HEBB_COUNT_SIM, HEBB_COUNT_NOISE = 0, 1  # tnf_hebb_launch_count
HEBB_MAX_N = 64  # include/tnf_hebb.h
EFN_COUNT_PRIOR, EFN_COUNT_NOISE, EFN_COUNT_KL = 0, 1, 2  # tnf_efn_launch_count
EFN_MAX_D, EFN_MAX_DF = 64, 1024  # include/tnf_efn.h
PADTRAIN_COUNT_EMBED_ROWS, PADTRAIN_COUNT_GATHER_ROWS, PADTRAIN_COUNT_EMBED_PARAMS = 0, 1, 2  # tnf_padtrain_launch_count
PADTRAIN_COUNT_GATHER_PARAMS, PADTRAIN_COUNT_BWD = 3, 4

_vp, _i32, _i64, _f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float

# name -> (restype, argtypes); kept in step with include/tnf.h (tests/test_cabi.py checks it)
SIGNATURES = {
    "tnf_version": (ctypes.c_int, []),
    "tnf_last_error": (ctypes.c_char_p, []),
    "tnf_set_option": (ctypes.c_int, [_i32, _i32]),
    "tnf_get_option": (ctypes.c_int, [_i32, _vp]),
    "tnf_diag_launch_count": (_i64, [_i32]),
    "tnf_set_launch_gate": (ctypes.c_int, [_vp]),
    "tnf_gated_copy_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "tnf_coupling_num_params": (_i64, [_i32, _i32, _i32, _i32]),
    "tnf_flow_num_params": (_i64, [_i32, _i32, _i32, _i32]),
    "tnf_has_fast_path": (ctypes.c_int, [_i32, _i32, _i32]),
    "tnf_coupling": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32,
                                    _i32, _i64, _i32, _vp]),
    "tnf_affine": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i64, _vp]),
    "tnf_bn_apply": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "tnf_bn_batch_workspace_bytes": (_i64, [_i32]),
    "tnf_bn_batch_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp, _i64, _vp]),
    "tnf_bn_batch_moments_f32": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "tnf_bn_batch_normalize_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _f32, _vp, _i64, _vp]),
    "tnf_bn_batch_backward_sums_f32": (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "tnf_bn_batch_backward_apply_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "tnf_coupling_backward": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                             _i32, _i32, _i32, _i64, _i64, _vp]),
    "tnf_coupling_backward_workspace_bytes": (_i64, [_i32, _i64, _i64, _i64, _i32, _i32, _i32, _i32]),
    "tnf_coupling_backward_ws": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                                _i32, _i32, _i32, _i64, _i64, _vp, _i64, _vp]),
    "tnf_maf_backward_workspace_bytes": (_i64, [_i32, _i64, _i64, _i64, _i32, _i32, _i32]),
    "tnf_maf_backward_ws": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                           _i32, _i64, _i64, _vp, _i64, _vp]),
    "tnf_affine_backward": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                           _i64, _i64, _vp]),
    "tnf_bn_apply_backward": (ctypes.c_int, [_i32, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "tnf_bn_batch_backward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _vp]),
    "tnf_cond_flow_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i32]),
    "tnf_cond_flow_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "tnf_cond_flow_log_prob_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32,
                                                   _i32, _i32, _i64, _i64, _vp, _i64, _vp]),
    "tnf_cond_flow_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32,
                                                  _i32, _i32, _i64, _i64, _vp, _i64, _vp]),
    "tnf_cond_flow_acts_floats": (_i64, [_i64, _i32, _i32, _i32]),
    "tnf_cond_flow_deltas_floats": (_i64, [_i64, _i32, _i32, _i32, _i32]),
    "tnf_cond_flow_bwd_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "tnf_cond_flow_log_prob_fwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32,
                                                       _i32, _i32, _i64, _i64, _vp, _i64, _vp]),
    "tnf_cond_flow_log_prob_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                                       _i64, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _vp,
                                                       _i64, _vp]),
    "tnf_ar_flow_supported": (ctypes.c_int, [_i32, _i32, _i32]),
    "tnf_ar_flow_workspace_bytes": (_i64, [_i64, _i32]),
    "tnf_ar_flow_log_prob_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                                 _i32, _i64, _vp, _i64, _vp]),
    "tnf_ar_flow_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                                _i64, _vp, _i64, _vp]),
    "tnf_to_interval": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "tnf_to_interval_backward": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "tnf_to_simplex": (ctypes.c_int, [_i32, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "tnf_to_simplex_backward": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "tnf_maf_num_params": (_i64, [_i32, _i32, _i32]),
    "tnf_maf": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i64, _vp]),
    "tnf_maf_backward": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                        _i32, _i64, _i64, _vp]),
    "tnf_base_log_density_f64": (ctypes.c_int, [_i32, _vp, _vp, _i64, _i32, _vp]),
    "tnf_flow_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32, _i32, _i32, _i32]),
    "tnf_flow_fused_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_flow_fused2_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_flow_fused3_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_flow_log_prob_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32,
                                             _i32, _i32, _i32, _i64, _i32, _vp, _i64, _vp]),
    "tnf_flow_log_prob_diag_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32,
                                                  _i32, _i32, _i32, _i64, _i32, _vp, _i64, _vp, _vp]),
    "tnf_flow_train_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32, _i32, _i32, _i32]),
    "tnf_flow_log_prob_fwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                                 _i32, _i64, _vp, _i64, _vp]),
    "tnf_flow_log_prob_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32,
                                                 _i32, _i32, _i32, _i64, _i64, _vp, _i64, _vp]),
    "tnf_flow_forward_batch_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "tnf_flow_forward_batch_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                                  _i32, _i64, ctypes.c_float, _vp, _i64, _vp]),
    "tnf_flow_forward_batch_begin_f32": (ctypes.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _i64, _vp, _i64, _vp]),
    "tnf_flow_forward_batch_layer_f32": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                                        _i32, _i64, _vp, _i64, _vp]),
    "tnf_flow_forward_batch_fold_f32": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i64,
                                                       ctypes.c_float, _vp, _i64, _vp]),
    "tnf_flow_forward_batch_end_f32": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _vp]),
    "tnf_flow_forward_train_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32, _i32, _i32]),
    "tnf_flow_forward_train_fwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                                      _i32, _i32, _i64, ctypes.c_float, _vp, _i64, _vp]),
    "tnf_flow_forward_train_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64,
                                                      _i32, _i32, _i32, _i32, _i64, _i64, _vp, _i64, _vp]),
    "tnf_maf_inverse_alpha": (ctypes.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i64,
                                             _vp]),
    "tnf_ar_flow_train_supported": (ctypes.c_int, [_i32, _i32, _i32]),
    "tnf_ar_flow_bwd_workspace_bytes": (_i64, [_i64, _i32]),
    "tnf_ar_flow_log_prob_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32,
                                                    _i32, _i32, _i64, _i64, _vp, _i64, _vp]),
    "tnf_flow_train_rev_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_flow_train_rev_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32, _i32, _i32, _i32]),
    "tnf_flow_log_prob_fwd_rev_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                                     _i32, _i32, _i64, _vp]),
    "tnf_flow_log_prob_bwd_rev_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32,
                                                     _i32, _i32, _i32, _i64, _i64, _vp, _i64, _vp, _vp]),
    "tnf_flow_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                            _i32, _i32, _i64, _i32, _vp, _i64, _vp]),
    "tnf_flow_forward_logq_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                                 _i32, _i32, _i64, _i32, _vp, _i64, _vp]),
    "tnf_flow_padded_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_flow_padded_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "tnf_flow_padded_log_prob_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                                    _i32, _i32, _i64, _vp, _i64, _vp, _vp]),
    "tnf_flow_padded_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                                   _i32, _i32, _i64, _vp, _i64, _vp]),
    "tnf_ef_num_eta": (_i32, [_i32, _i32]),
    "tnf_ef_suffstats": (ctypes.c_int, [_i32, _i32, _vp, _vp, _i64, _i32, _vp]),
    "tnf_ef_suffstats_backward": (ctypes.c_int, [_i32, _i32, _vp, _vp, _vp, _i64, _i32, _vp]),
    "tnf_ef_launch_count": (_i64, [_i32]),
    "tnf_ef_dot_supported": (ctypes.c_int, [_i32, _i32]),
    "tnf_ef_dot": (ctypes.c_int, [_i32, _i32, _vp, _vp, _vp, _i64, _i64, _i32, _i64, _vp]),
    "tnf_ef_dot_bwd_workspace_bytes": (_i64, [_i32, _i64, _i64, _i32]),
    "tnf_ef_dot_backward": (ctypes.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i64, _vp, _i64, _vp]),
}

# the mixture-of-Gaussians family, declared in include/tnf_mog.h: a table of its own, because every entry of SIGNATURES
# has its rows in the pinned host tables of tnf.h (tests/test_mog_host.py keeps this one in step with its header)
MOG_SIGNATURES = {
    "tnf_mog_num_params": (_i64, [_i32, _i32]),
    "tnf_mog_supported": (ctypes.c_int, [_i32, _i32]),
    "tnf_mog_launch_count": (_i64, [_i32]),
    "tnf_mog_log_prob_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i64, _vp]),
    "tnf_mog_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32, _i32]),
    "tnf_mog_log_prob_backward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i64,
                                                      _vp, _i64, _vp]),
    "tnf_mog_sample_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i64, _vp]),
}

# the rejection-ABC family, declared in include/tnf_abc.h: again a table of its own (tests/test_abc_host.py)
ABC_SIGNATURES = {
    "tnf_abc_supported": (ctypes.c_int, [_i32]),
    "tnf_abc_launch_count": (_i64, [_i32]),
    "tnf_abc_smc_mat_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp]),
    "tnf_abc_propose_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _vp]),
    "tnf_abc_noise_f32": (ctypes.c_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp]),
}

# the Hebbian learning-rule simulator, declared in include/tnf_hebb.h: a fourth table (tests/test_hebb_host.py)
HEBB_SIGNATURES = {
    "tnf_hebb_supported": (ctypes.c_int, [_i32]),
    "tnf_hebb_launch_count": (_i64, [_i32]),
    "tnf_hebb_simulate_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32,
                                             _i64, _i64, _f32, _vp]),
    "tnf_hebb_noise_f32": (ctypes.c_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _vp]),
}

# the EFN training loop's prior and KL kernels, declared in include/tnf_efn.h: a fifth table (tests/test_efn_host.py)
EFN_SIGNATURES = {
    "tnf_efn_supported": (ctypes.c_int, [_i32, _i32]),
    "tnf_efn_launch_count": (_i64, [_i32]),
    "tnf_efn_prior_num_noise": (_i64, [_i32, _i32, _i32]),
    "tnf_efn_prior_noise_f32": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, _i64, _i64, _i64, _vp]),
    "tnf_efn_prior_f32": (ctypes.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _f32, _i64, _i64, _i64, _i64, _vp]),
    "tnf_efn_kl_workspace_bytes": (_i64, [_i32, _i64, _i64, _i32]),
    "tnf_efn_kl_f32": (ctypes.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i64, _i64, _i32, _vp, _i64, _vp]),
}

# training a coupling flow of any width 2 .. 63 through the reversible backward at the embedded width, declared in
# include/tnf_padtrain.h: a sixth table (tests/test_padded_train_host.py)
PADTRAIN_SIGNATURES = {
    "tnf_flow_padded_train_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_flow_padded_width": (ctypes.c_int, [_i32]),
    "tnf_flow_padded_embed_index": (_i64, [_i32, _i32, _i32, _i32, _i64]),
    "tnf_padtrain_launch_count": (_i64, [_i32]),
    "tnf_flow_padded_embed_rows_f32": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "tnf_flow_padded_gather_rows_f32": (ctypes.c_int, [_vp, _vp, _i64, _i32, _vp]),
    "tnf_flow_padded_embed_params_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i64,
                                                        _vp]),
    "tnf_flow_padded_gather_params_f32": (ctypes.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i64, _vp]),
    "tnf_flow_padded_train_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32, _i32, _i32, _i32]),
    "tnf_flow_padded_log_prob_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32,
                                                        _i32, _i32, _i64, _i64, _vp, _i64, _vp, _vp]),
}

# sampling a coupling flow of any width 2 .. 63 with fresh batch statistics in one call (the batch-statistics chains at
# the embedded width with a pad-aware fold), declared in include/tnf_padbatch.h: a seventh table
# (tests/test_padded_batch_host.py)
PADBATCH_SIGNATURES = {
    "tnf_flow_padded_batch_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_padbatch_launch_count": (_i64, [_i32]),
    "tnf_flow_padded_batch_fold_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i64, _i64, _i32, _i32, _f32,
                                                      _vp]),
    "tnf_flow_padded_batch_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32, _i32, _i32, _i32]),
    "tnf_flow_padded_forward_batch_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                                         _i32, _i64, _f32, _vp, _i64, _vp]),
    "tnf_flow_padded_batch_train_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32, _i32, _i32, _i32]),
    "tnf_flow_padded_forward_train_fwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32,
                                                             _i32, _i32, _i32, _i64, _f32, _vp, _i64, _vp]),
    "tnf_flow_padded_forward_train_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                                                             _i64, _i32, _i32, _i32, _i32, _i64, _i64, _vp, _i64, _vp]),
}

# per-context coupling flows with fewer than 32 samples per context, one launch per call, declared in
# include/tnf_ctxflow.h: an eighth table (tests/test_ctx_flow_host.py)
CTXFLOW_SIGNATURES = {
    "tnf_ctx_flow_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i64]),
    "tnf_ctx_flow_launch_count": (_i64, [_i32]),
    "tnf_ctx_flow_log_prob_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32,
                                                 _i64, _vp]),
    "tnf_ctx_flow_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i64, _vp]),
}

# the log_prob backward of those per-context flows, one launch per call, declared in include/tnf_ctxtrain.h: a ninth
# table (tests/test_ctx_train_host.py)
CTXTRAIN_SIGNATURES = {
    "tnf_ctx_train_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i64]),
    "tnf_ctx_train_launch_count": (_i64, []),
    "tnf_ctx_train_log_prob_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32,
                                                      _i64, _i64, _vp]),
}

# training through frozen-statistics sampling: the backward of the sampling pass in one walk kernel, declared in
# include/tnf_sampletrain.h: a tenth table (tests/test_sample_train_host.py)
SAMPLETRAIN_SIGNATURES = {
    "tnf_flow_sample_train_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_flow_sample_train_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32, _i32, _i32, _i32]),
    "tnf_sampletrain_launch_count": (_i64, []),
    "tnf_flow_sample_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                               _i32, _i64, _i64, _vp, _i64, _vp, _vp]),
}

# training an autoregressive flow through its samples: the MAF sampling backward in one kernel, alone and with the
# frozen-statistics stack folded in, declared in include/tnf_arsample.h: an eleventh table (tests/test_arsample_host.py)
ARSAMPLE_SIGNATURES = {
    "tnf_maf_sample_bwd_supported": (ctypes.c_int, [_i32, _i32, _i32]),
    "tnf_arsample_launch_count": (_i64, []),
    "tnf_maf_sample_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i64,
                                              _i64, _vp]),
    "tnf_ar_flow_sample_bwd_workspace_bytes": (_i64, [_i64, _i32]),
    "tnf_ar_flow_sample_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                                  _i64, _i64, _vp, _i64, _vp]),
}

# sampling an autoregressive flow with fresh batch statistics, one call each way, declared in include/tnf_arbatch.h: a
# twelfth table (tests/test_arbatch_host.py)
ARBATCH_SIGNATURES = {
    "tnf_ar_flow_batch_supported": (ctypes.c_int, [_i32, _i32, _i32]),
    "tnf_ar_flow_batch_train_supported": (ctypes.c_int, [_i32, _i32, _i32]),
    "tnf_arbatch_launch_count": (_i64, [_i32]),
    "tnf_ar_flow_forward_batch_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32]),
    "tnf_ar_flow_forward_batch_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                                     _i64, _f32, _vp, _i64, _vp]),
    "tnf_ar_flow_batch_bwd_workspace_bytes": (_i64, [_i64, _i64, _i64, _i32]),
    "tnf_ar_flow_batch_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                                 _i64, _i64, _vp, _i64, _vp]),
}

# training per-context flows with fewer than 32 samples each through their frozen-statistics samples: the backward of
# tnf_ctx_flow_forward_f32 in one launch, declared in include/tnf_ctxsample.h: a thirteenth table
# (tests/test_ctx_sample_host.py)
CTXSAMPLE_SIGNATURES = {
    "tnf_ctx_sample_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i64]),
    "tnf_ctx_sample_launch_count": (_i64, []),
    "tnf_ctx_sample_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32,
                                              _i64, _i64, _vp]),
}

# the whole coupling flow in one launch at 17 <= num_units <= 64 and any 2 <= D <= 64, declared in
# include/tnf_wideflow.h: a fourteenth table (tests/test_wideflow_host.py)
WIDEFLOW_SIGNATURES = {
    "tnf_wide_flow_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_wide_flow_launch_count": (_i64, [_i32]),
    "tnf_wide_flow_log_prob_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32,
                                                  _i64, _vp]),
    "tnf_wide_flow_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32,
                                                 _i64, _vp]),
}

# per-context coupling flows with fewer than 32 samples per context at 17 <= num_units <= 64, one launch per call each
# way (inference and the log_prob backward), declared in include/tnf_ctxwide.h: a fifteenth table
# (tests/test_ctx_wide_host.py)
CTXWIDE_SIGNATURES = {
    "tnf_ctx_wide_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i64]),
    "tnf_ctx_wide_train_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i64]),
    "tnf_ctx_wide_lds_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32, _i64]),
    "tnf_ctx_wide_launch_count": (_i64, [_i32]),
    "tnf_ctx_wide_log_prob_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32,
                                                 _i64, _vp]),
    "tnf_ctx_wide_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i64, _vp]),
    "tnf_ctx_wide_log_prob_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32,
                                                     _i64, _i64, _vp]),
}

# the same layout trained through its frozen-statistics samples: the backward of tnf_ctx_wide_forward_f32 in one launch,
# with a process-wide override of the workgroup's team size, declared in include/tnf_ctxwidesample.h
# (tests/test_ctx_wide_sample_host.py).  Not a `*_SIGNATURES` table: those are a closed set of fifteen
CTXWIDESAMPLE_ENTRIES = {
    "tnf_ctx_wide_sample_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i64]),
    "tnf_ctx_wide_sample_launch_count": (_i64, []),
    "tnf_ctx_wide_sample_waves": (ctypes.c_int, [_i32, _i32, _i64]),
    "tnf_ctx_wide_sample_set_waves": (ctypes.c_int, [_i32]),
    "tnf_ctx_wide_sample_bwd_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32,
                                                   _i32, _i64, _i64, _vp]),
}

# the whole coupling flow at 17 <= num_units <= 64 with any number of stages, one layer's operand image streamed through
# LDS at a time, declared in include/tnf_widestream.h (tests/test_wide_stream_host.py).  Not a `*_SIGNATURES` table
# either, for the same reason
WIDESTREAM_ENTRIES = {
    "tnf_wide_flow_stream_supported": (ctypes.c_int, [_i32, _i32, _i32, _i32]),
    "tnf_wide_flow_stream_lds_bytes": (_i64, [_i32, _i32, _i32]),
    "tnf_wide_flow_stream_tiles": (ctypes.c_int, [_i32, _i32, _i32, _i32, _i64, _i64]),
    "tnf_wide_flow_stream_set_tiles": (ctypes.c_int, [_i32]),
    "tnf_wide_flow_stream_launch_count": (_i64, [_i32]),
    "tnf_wide_flow_stream_log_prob_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32,
                                                         _i32, _i64, _vp]),
    "tnf_wide_flow_stream_forward_f32": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32,
                                                        _i64, _vp]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "torch_nf_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C torch_nf_amd/csrc` (hipcc, --offload-arch=gfx950). "
            "There is no non-HIP fallback." % LIB_PATH
        )
    lib = ctypes.CDLL(LIB_PATH)
    for table in (SIGNATURES, MOG_SIGNATURES, ABC_SIGNATURES, HEBB_SIGNATURES, EFN_SIGNATURES, PADTRAIN_SIGNATURES,
                  PADBATCH_SIGNATURES, CTXFLOW_SIGNATURES, CTXTRAIN_SIGNATURES, SAMPLETRAIN_SIGNATURES, ARSAMPLE_SIGNATURES,
                  ARBATCH_SIGNATURES, CTXSAMPLE_SIGNATURES, WIDEFLOW_SIGNATURES, CTXWIDE_SIGNATURES,
                  CTXWIDESAMPLE_ENTRIES, WIDESTREAM_ENTRIES):
        for name, (res, args) in table.items():
            fn = getattr(lib, name)  # AttributeError here = header / library out of step
            fn.restype = res
            fn.argtypes = args
    return lib


lib = _load()


class TnfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libtnf_hip error %d: %s" % (code, msg))
        self.code = code


def check(rc):
    if rc < 0:
        raise TnfError(rc, lib.tnf_last_error().decode("utf-8", "replace"))
    return rc


_OPTION_KEYS = (OPT_FORCE_GENERIC, OPT_FLOW_VARIANT, OPT_LAYER_VARIANT, OPT_COND_VARIANT, OPT_TRAIN_BWD_FP32,
                OPT_OPERAND_PREC, OPT_REV_VARIANT)


def options_snapshot():
    """The calling thread's tnf_set_option values (options are thread-local in the library)."""
    out = []
    val = ctypes.c_int32(0)
    for key in _OPTION_KEYS:
        check(lib.tnf_get_option(key, ctypes.addressof(val)))
        out.append(val.value)
    return tuple(out)


@contextlib.contextmanager
def option_set(key, value, restore=None):
    """`with option_set(key, value)`: one thread-local option set for a block, its previous value back afterwards
    (`restore`: that value, from a caller that keeps track of it itself)."""
    if restore is None:
        before = ctypes.c_int32(0)
        check(lib.tnf_get_option(key, ctypes.addressof(before)))
        restore = before.value
    check(lib.tnf_set_option(key, value))
    try:
        yield
    finally:
        check(lib.tnf_set_option(key, restore))


class options_reentered(object):
    """`with options_reentered(snapshot)`: run a block under the options another thread had.  autograd calls
    Function.backward on its own device thread, where every option is still at its default: the Functions in ops.py
    record options_snapshot() in forward and re-enter it in backward, so a kernel variant chosen for a training step
    (TNF_OPT_TRAIN_BWD_FP32, TNF_OPT_FORCE_GENERIC, the operand precision) governs both of its halves."""

    def __init__(self, snapshot):
        self.snapshot = snapshot

    def __enter__(self):
        self.before = options_snapshot()
        if self.before != self.snapshot:
            for key, value in zip(_OPTION_KEYS, self.snapshot):
                check(lib.tnf_set_option(key, value))

    def __exit__(self, *exc):
        if self.before != self.snapshot:
            for key, value in zip(_OPTION_KEYS, self.before):
                lib.tnf_set_option(key, value)
        return False


def require_device():
    """The product path is HIP only: fail loudly when no GPU is visible."""
    if not torch.cuda.is_available():
        raise RuntimeError(
            "torch_nf_amd needs a HIP device (MI355X / gfx950): torch.cuda.is_available() is False "
            "and there is deliberately no CPU implementation of the flow kernels."
        )
    return torch.device("cuda", torch.cuda.current_device())


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream

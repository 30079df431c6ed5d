"""ctypes binding of the C-ABI in ``include/cmbpo_hip.h`` (libcmbpo_hip.so).

This is the stub a maintainer of the reference would add:
the reference has no FFI of its own, its hot path is TF ``sess.run`` + NumPy.
The library is built in-tree by ``__graft_entry__.build()``; if it is missing
the import of any product module fails loudly -- there is no CPU fallback.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcmbpo_hip.so")

ACT_SWISH, ACT_TANH = 0, 1
HEAD_PROB, HEAD_DETMEAN, HEAD_GAUSS_PI = 0, 1, 2
LOSS_DEFAULT, LOSS_NLL = 0, 1      # cmbpo_trainer_set_loss
ENS_FP32, ENS_SPLIT_BF16, ENS_SPLIT_F16 = 0, 1, 2    # cmbpo_set_ens_matrix_path
TASK_DEFAULT, TASK_HCS, TASK_ANTSAFE = 0, 1, 2
TASK_LEARNED_COST = 0x100     # CMBPO_TASK_LEARNED_COST: flag bit or-ed into a rule id (learned cost head)
TASK_USER_BASE, TASK_USER_SLOTS = 16, 64     # CMBPO_TASK_USER_BASE / _SLOTS: ids of registered rule tables (cmbpo_amd.statics)
RULE_MAX_CLAUSES = 16
RULE_HEALTHY, RULE_FATAL, RULE_COST = 0, 1, 2                     # clause roles
RULE_SRC_NEXT_OBS, RULE_SRC_OBS, RULE_SRC_ACT = 0, 1, 2           # clause sources
RULE_ABS, RULE_LO_STRICT, RULE_HI_STRICT, RULE_ANY = 1, 2, 4, 8   # clause flags

# models/statics.py:56-69 -- task name -> rule id (statics.register_task adds the names of registered rule tables)
TASK_IDS = {
    "default": TASK_DEFAULT,
    "HalfCheetah-v2": TASK_DEFAULT,
    "HalfCheetahSafe-v2": TASK_HCS,
    "AntSafe-v2": TASK_ANTSAFE,
}

_p = C.c_void_p
_i = C.c_int
_sz = C.c_size_t

# name -> (restype, argtypes); every symbol include/cmbpo_hip.h declares.
SIGNATURES = {
    "cmbpo_last_error": (C.c_char_p, []),
    "cmbpo_version": (_i, []),
    "cmbpo_set_ens_matrix_path": (_i, [_i]),
    "cmbpo_get_ens_matrix_path": (_i, []),
    "cmbpo_set_ens_f16_min_rows": (_i, [_i]),
    "cmbpo_set_ens_f16_row_tiles": (_i, [_i]),
    "cmbpo_set_ens_f16_image_min_rows": (_i, [_i]),
    "cmbpo_mlp_create": (_i, [C.POINTER(_p), _i, _i, _i, _i, _i, _i]),
    "cmbpo_mlp_destroy": (None, [_p]),
    "cmbpo_mlp_load": (_i, [_p] * 13),
    "cmbpo_mlp_load_policy_flat": (_i, [_p, _p, _p]),
    "cmbpo_ens_forward": (_i, [_p, _p, _i, _p, _i, _p, _p, _i, _i, _p, _p, _p]),
    "cmbpo_ens_predict_mean": (_i, [_p, _p, _i, _p, _p, _i, _p, _p]),
    "cmbpo_critic_pair_supported": (_i, [_p, _p]),
    "cmbpo_critic_pair_predict": (_i, [_p, _p, _p, _i, _p, _p, _i, _p, _p, _p]),
    "cmbpo_critic_pair_predict_var": (_i, [_p, _p, _p, _i, _p, _p, _i, C.c_float, C.c_float, _p, _p, _p, _p, _p]),
    "cmbpo_policy_forward": (_i, [_p, _p, _i, _p, _p, _p, _i, _p, _p, _p, _p, _p]),
    "cmbpo_fakeenv_post": (_i, [_i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i,
                                _p, _p, _p, _p, _p, _p, _p, _p]),
    "cmbpo_fakeenv_post_noise": (_i, [_i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i,
                                      _p, _p, _p, _p, _p, _p, _p, _p, _p]),
    "cmbpo_fakeenv_post_disagreement": (_i, [_i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i,
                                             _p, _p, _p, _p, _p, _p, _p, _p, C.c_float, C.c_float, _p, _p, _p]),
}



class RuleClauseStruct(C.Structure):
    """ctypes image of ``cmbpo_rule_clause_t`` (32 bytes)."""
    _fields_ = [(n, C.c_int32) for n in ("role", "src", "col0", "n_cols", "flags")] + \
               [(n, C.c_float) for n in ("scale", "lo", "hi")]


class TaskRulesStruct(C.Structure):
    """ctypes image of ``cmbpo_task_rules_t`` (528 bytes)."""
    _fields_ = [(n, C.c_int32) for n in ("n_clauses", "require_finite", "cost_on_term", "reserved")] + \
               [("clause", RuleClauseStruct * RULE_MAX_CLAUSES)]


SIGNATURES.update({
    "cmbpo_task_rules_register": (_i, [C.POINTER(TaskRulesStruct), C.POINTER(C.c_int)]),
    "cmbpo_task_rules_get": (_i, [_i, C.POINTER(TaskRulesStruct)]),
    "cmbpo_task_rules_count": (_i, []),
})

RULE_SRC_DERIVED = 3                              # CMBPO_RULE_SRC_DERIVED: a clause over derived quantities
RULE_MAX_DERIVED, RULE_MAX_TERMS = 8, 4           # CMBPO_RULE_MAX_DERIVED / _TERMS


class RuleTermStruct(C.Structure):
    """ctypes image of ``cmbpo_rule_term_t`` (16 bytes)."""
    _fields_ = [("src", C.c_int16), ("pow", C.c_int16), ("col", C.c_int32), ("w", C.c_float), ("c", C.c_float)]


class RuleDerivedStruct(C.Structure):
    """ctypes image of ``cmbpo_rule_derived_t`` (80 bytes)."""
    _fields_ = [("n_terms", C.c_int32), ("bias", C.c_float), ("reserved", C.c_int32 * 2), ("term", RuleTermStruct * RULE_MAX_TERMS)]


class RuleDerivedTableStruct(C.Structure):
    """ctypes image of ``cmbpo_rule_derived_table_t`` (656 bytes)."""
    _fields_ = [("n_derived", C.c_int32), ("reserved", C.c_int32 * 3), ("derived", RuleDerivedStruct * RULE_MAX_DERIVED)]


SIGNATURES.update({
    "cmbpo_task_rules_register_ex": (_i, [C.POINTER(TaskRulesStruct), C.POINTER(RuleDerivedTableStruct), C.POINTER(C.c_int)]),
    "cmbpo_task_rules_get_derived": (_i, [_i, C.POINTER(RuleDerivedTableStruct)]),
})


class RolloutStruct(C.Structure):
    """ctypes image of ``cmbpo_rollout_t`` (include/cmbpo_hip.h), field for field."""
    _fields_ = (
        [(n, C.c_int32) for n in ("B", "T", "obs_dim", "act_dim", "max_path_length", "ptr",
                                  "uncertainty_mode", "rank", "world")]
        + [("max_samples", C.c_int64), ("dkl_lim", C.c_double), ("gamma", C.c_double), ("lam", C.c_double),
           ("cost_gamma", C.c_double), ("cost_lam", C.c_double)]
        + [(n, C.c_void_p) for n in ("alive_idx", "alive_idx_out", "iscal", "dscal")]
        + [("use_host_budget", C.c_int32), ("host_rank_off", C.c_int32), ("host_excess", C.c_int64)]
        + [(n, C.c_void_p) for n in (
            "alive", "fin_code", "len",
            "cur_obs", "next_obs", "act_t", "logp_t", "mu_t", "ls_t", "v_t", "vc_t", "v_n", "vc_n",
            "rew_t", "cost_t", "dkl_t", "epv_t", "term_t",
            "dkl_acc", "path_ret", "path_cost", "path_dyn_var", "store_part",
            "obs_buf", "act_buf", "mu_buf", "ls_buf",
            "rew_buf", "val_buf", "cost_buf", "cval_buf", "logp_buf",
            "adv_buf", "ret_buf", "cadv_buf", "cret_buf",
            "xi")]                      # stochastic transitions: NULL = off
        + [("xi_stride", C.c_int64)]
    )


# iscal / dscal slots (CMBPO_I_* / CMBPO_D_* in the header)
I_N_ALIVE, I_N_UNC, I_N_FIN_PRE, I_N_STORED, I_N_ALIVE_OUT, I_SIZE, I_N_FIN_POST = 0, 1, 2, 3, 4, 5, 6
(D_TOTAL_SAMPLES, D_TOTAL_COST, D_TOTAL_REW, D_TOTAL_VS, D_TOTAL_CVS, D_TOTAL_DKL, D_TOTAL_DYN_EP_VAR,
 D_MAX_DKL, D_MAX_PATH_RETURN, D_DKL_SUM_T, D_STEP_MAX_DKL, D_SUM_PATH_RET, D_SUM_PATH_COST) = range(13)
D_TOTAL_REW_VAR, D_TOTAL_COST_VAR = 13, 14      # ensemble disagreement on reward / cost, summed over the stored rows
D_TOTAL_V_VAR, D_TOTAL_VC_VAR = 15, 16          # critic disagreement (member variance of V / VC), summed over the stored rows

_rp = C.POINTER(RolloutStruct)
SIGNATURES.update({
    "cmbpo_rollout_reset": (_i, [_rp, _p]),
    "cmbpo_rollout_decide": (_i, [_rp, _p]),
    "cmbpo_rollout_count": (_i, [_rp, _p]),
    "cmbpo_rollout_finish": (_i, [_rp, _i, _p]),
    "cmbpo_rollout_store": (_i, [_rp, _p]),
    "cmbpo_rollout_book_pre_max_rows": (_i, []),
    "cmbpo_rollout_book_pre": (_i, [_rp, _i, _p]),
    "cmbpo_rollout_book_post": (_i, [_rp, _i, _p]),
    "cmbpo_rollout_read_scalars": (_i, [_rp, _p, _p]),
    "cmbpo_rollout_compact": (_i, [_rp, _p]),
    "cmbpo_rollout_step": (_i, [_rp, _i, _p, _p, _p, _p, _i, _i, _p, _p, _p, _p, _p]),
    "cmbpo_rollout_run": (_i, [_rp, _i, _p, _p, _p, _p, _i, _i, _p, _p, C.c_long, C.c_long, _p, _p, _i, C.c_double, _i, _p,
                               C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), _p]),
    "cmbpo_buffer_offsets": (_i, [_rp, _p, _p]),
    "cmbpo_buffer_moments": (_i, [_rp, _i, _p, _p]),
    "cmbpo_buffer_prepare": (_i, [_rp, _p, _p, _p]),
    "cmbpo_buffer_flatten": (_i, [_rp, _p, _p, C.POINTER(C.c_void_p), _p]),
    "cmbpo_buffer_trust_weights": (_i, [_rp, _p, C.c_double, _p, _p]),
})


class IvGaeStruct(C.Structure):
    """ctypes image of ``cmbpo_iv_gae_t``: the arrays of the inverse-variance-weighted GAE that travel beside the rollout struct."""
    _fields_ = [(n, C.c_void_p) for n in ("cumvar_buf", "lam_vec", "lam_pow", "clam_vec", "clam_pow")] + [("eps", C.c_double)]


SIGNATURES.update({
    "cmbpo_rollout_iv_attach": (_i, [_rp, C.POINTER(IvGaeStruct)]),
    "cmbpo_rollout_iv_detach": (_i, [_rp]),
})


class DisagreementStruct(C.Structure):
    """ctypes image of ``cmbpo_disagreement_t``: the pessimism coefficients and the arrays of the ensemble disagreement on
    reward and cost that travel beside the rollout struct."""
    _fields_ = [("kappa_rew", C.c_float), ("kappa_cost", C.c_float)] + \
               [(n, C.c_void_p) for n in ("rew_var_t", "cost_var_t", "path_rew_var", "path_cost_var", "part")]


SIGNATURES.update({
    "cmbpo_rollout_disagreement_attach": (_i, [_rp, C.POINTER(DisagreementStruct)]),
    "cmbpo_rollout_disagreement_detach": (_i, [_rp]),
})


class ValueDisagreementStruct(C.Structure):
    """ctypes image of ``cmbpo_value_disagreement_t``: the pessimism coefficients and the arrays of the critics' own
    disagreement that travel beside the rollout struct."""
    _fields_ = [("kappa_v", C.c_float), ("kappa_vc", C.c_float)] + [(n, C.c_void_p) for n in ("v_var", "vc_var", "part")]


SIGNATURES.update({
    "cmbpo_rollout_value_disagreement_attach": (_i, [_rp, C.POINTER(ValueDisagreementStruct)]),
    "cmbpo_rollout_value_disagreement_detach": (_i, [_rp]),
})



TERM_ELITE, TERM_ANY, TERM_MAJORITY = 0, 1, 2     # CMBPO_TERM_*: whose vote ends a branch (learned termination head)
TERM_MEMBERS = {"elite": TERM_ELITE, "any": TERM_ANY, "majority": TERM_MAJORITY}


class TermHeadStruct(C.Structure):
    """ctypes image of ``cmbpo_term_head_t`` (24 bytes): threshold and vote of the learned termination head, and its two
    optional per-row outputs."""
    _fields_ = [("threshold", C.c_float), ("members", C.c_int32), ("term_pred", C.c_void_p), ("term_votes", C.c_void_p)]


_tp = C.POINTER(TermHeadStruct)
SIGNATURES.update({
    "cmbpo_fakeenv_post_term": (_i, [_i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i,
                                     _p, _p, _p, _p, _p, _p, _p, _p, C.c_float, C.c_float, _p, _p, _tp, _p]),
    "cmbpo_rollout_term_head_attach": (_i, [_rp, _tp]),
    "cmbpo_rollout_term_head_detach": (_i, [_rp]),
})


COST_MAGNITUDE, COST_LOGISTIC = 0, 1     # CMBPO_COST_*: how the learned-cost column is read
COST_KINDS = {"gaussian": COST_MAGNITUDE, "logistic": COST_LOGISTIC}


class CostHeadStruct(C.Structure):
    """ctypes image of ``cmbpo_cost_head_t`` (16 bytes): the reading of the learned-cost column, the shift that undoes a class
    weight, and the optional per-row output of the elite's raw logit."""
    _fields_ = [("kind", C.c_int32), ("logit_shift", C.c_float), ("cost_logit", C.c_void_p)]


_chp = C.POINTER(CostHeadStruct)
SIGNATURES.update({
    "cmbpo_fakeenv_post_cost": (_i, [_i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i,
                                     _p, _p, _p, _p, _p, _p, _p, _p, C.c_float, C.c_float, _p, _p, _tp, _chp, _p]),
    "cmbpo_rollout_cost_head_attach": (_i, [_rp, _chp]),
    "cmbpo_rollout_cost_head_detach": (_i, [_rp]),
})

# sampled terminations: a threshold per row in place of the head's scalar (thresholds: utils.term_thresholds)
SIGNATURES.update({
    "cmbpo_fakeenv_post_term_draws": (_i, [_i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i,
                                           _p, _p, _p, _p, _p, _p, _p, _p, C.c_float, C.c_float, _p, _p, _tp, _chp, _p, _p]),
    "cmbpo_rollout_term_draws_attach": (_i, [_rp, _p, C.c_long]),
})


VOTE_MEAN = 3                                     # CMBPO_VOTE_MEAN: the expected indicator votes / E (the static cost only)
RULE_DONE_MEMBERS = TERM_MEMBERS                  # whose vote ends a branch by the task's static termination rule
RULE_COST_MEMBERS = dict(TERM_MEMBERS, mean=VOTE_MEAN)     # ... and whose vote a step costs by its static cost rule


class RuleVotesStruct(C.Structure):
    """ctypes image of ``cmbpo_rule_votes_t`` (24 bytes): the votes of the ensemble-voted static rules and their two optional
    per-row outputs."""
    _fields_ = [("done_members", C.c_int32), ("cost_members", C.c_int32), ("done_votes", C.c_void_p), ("cost_votes", C.c_void_p)]


_rvp = C.POINTER(RuleVotesStruct)
SIGNATURES.update({
    "cmbpo_fakeenv_post_votes": (_i, [_i, _i, _i, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i,
                                      _p, _p, _p, _p, _p, _p, _p, _p, C.c_float, C.c_float, _p, _p, _tp, _chp, _p, _rvp, _p]),
    "cmbpo_rollout_rule_votes_attach": (_i, [_rp, _rvp]),
    "cmbpo_rollout_rule_votes_detach": (_i, [_rp]),
})


class PiBatchStruct(C.Structure):
    """ctypes image of ``cmbpo_pi_batch_t``."""
    _fields_ = [("n", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32)] + \
               [(k, C.c_void_p) for k in ("obs", "act", "adv", "cadv", "logp_old", "cost", "mu_old", "logstd_old")]


_bp = C.POINTER(PiBatchStruct)
SIGNATURES.update({
    "cmbpo_pi_create": (_i, [C.POINTER(_p), _i, _i, _i]),
    "cmbpo_pi_destroy": (None, [_p]),
    "cmbpo_pi_num_params": (_i, [_p]),
    "cmbpo_pi_set_params": (_i, [_p, _p, _p]),
    "cmbpo_pi_loss_grad": (_i, [_p, _bp, _i, _p, _p, _p]),
    "cmbpo_pi_fvp": (_i, [_p, _bp, _p, _p, _p]),
    "cmbpo_pi_keep_activations": (_i, [_p, _i]),
    "cmbpo_pi_saved_activation_uses": (C.c_long, [_p]),
    "cmbpo_pi_last_grid": (_i, [_p]),
    "cmbpo_pi_set_sample_weights": (_i, [_p, _p, _i, _p]),
    "cmbpo_set_pi_matrix_path": (None, [_i]),
    "cmbpo_get_pi_matrix_path": (_i, []),
    "cmbpo_pi_eval": (_i, [_p, _bp, _p, _p]),
    "cmbpo_cg_init": (_i, [_i, _p, _p, _p, _p, _p, _p]),
    "cmbpo_cg_step": (_i, [_i, _p, C.c_double, C.c_float, _p, _p, _p, _p, _p]),
    "cmbpo_pi_cg_solve": (_i, [_p, _bp, _p, C.c_double, C.c_float, _i, _p, _p, _p, _p, _p, _i, _p]),
    "cmbpo_pi_cg_release": (None, [_p]),
    "cmbpo_pi_cg_iter": (_i, [_p, _bp, C.c_double, C.c_float, _p, _p, _p, _p, _p]),
    "cmbpo_pi_cg_commit": (_i, [_p, _p]),
    "cmbpo_pi_cg_graph_launches": (C.c_long, []),
    "cmbpo_pi_cg_graph_captures": (C.c_long, []),
    "cmbpo_vec_lincomb": (_i, [_i, C.c_float, _p, C.c_float, _p, _p, _p]),
    "cmbpo_vec_dots": (_i, [_i, _i, C.POINTER(_p), C.POINTER(_p), _p, _p]),
    "cmbpo_gae_segments": (_i, [_i] + [_p] * 8 + [C.c_double] * 4 + [_p] * 5),
    "cmbpo_adv_normalize": (_i, [_i, _p, _p, _p, _p]),
})


class PiPpoCfgStruct(C.Structure):
    """ctypes image of ``cmbpo_pi_ppo_cfg_t``."""
    _fields_ = [("clip_ratio", C.c_float), ("clipped_adv", C.c_int32), ("objective_penalized", C.c_int32),
                ("ent_reg", C.c_float), ("pi_lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("adam_eps", C.c_float), ("target_kl", C.c_float), ("kl_margin", C.c_float)]


# slots of the first-order loop's state block (doubles; the layout is documented in the header)
PPO_STATE_DOUBLES = 32
(PPO_ST_STOP, PPO_ST_ITERS, PPO_ST_KL, PPO_ST_ADAM_T, PPO_ST_PEN_PARAM, PPO_ST_PEN_M, PPO_ST_PEN_V, PPO_ST_PEN_T,
 PPO_ST_PENALTY, PPO_ST_CR, PPO_ST_CC, PPO_ST_PRE) = range(12)
PPO_ST_POST = PPO_ST_PRE + 8
PPO_ST_CLIP = 27

_cp = C.POINTER(PiPpoCfgStruct)
SIGNATURES.update({
    "cmbpo_pi_ppo_grad": (_i, [_p, _bp, _cp, _p, _p, _p, _p]),
    "cmbpo_vec_adam_step": (_i, [_i, _p, _p, _p, _p, _p, C.c_float, C.c_float, C.c_float, C.c_float, _p]),
    "cmbpo_ppo_penalty_step": (_i, [_p, _p, C.c_double, C.c_double, C.c_double, _i, _p]),
    "cmbpo_pi_ppo_run": (_i, [_p, _bp, _cp, _p, _p, _p, _p, _i, _p]),
})

# ensemble training (csrc/ens_train.hip)
SIGNATURES.update({
    "cmbpo_trainer_create": (_i, [C.POINTER(_p), _p, _i, C.c_float, _p]),
    "cmbpo_trainer_destroy": (None, [_p]),
    "cmbpo_trainer_set_loss": (_i, [_p, _i]),
    "cmbpo_trainer_set_weights": (_i, [_p] * 8),
    "cmbpo_trainer_get_weights": (_i, [_p] * 8),
    "cmbpo_trainer_reset_optimizer": (_i, [_p, _p]),
    "cmbpo_trainer_get_moments": (_i, [_p, _i] + [_p] * 7),
    "cmbpo_trainer_set_moments": (_i, [_p, _i] + [_p] * 6 + [C.c_long, _p]),
    "cmbpo_mlp_set_scalers": (_i, [_p] * 6),
    "cmbpo_trainer_step": (_i, [_p, _p, _i, _p, _i, _p, _i, _i, _p]),
    "cmbpo_trainer_epoch": (_i, [_p, _p, _i, _p, _i, _p, _i, _i, _i, _p]),
    "cmbpo_trainer_losses": (_i, [_p, _p, _i, _p, _i, _p, _i, _i, _p, _p]),
    "cmbpo_trainer_steps_done": (C.c_long, [_p]),
    "cmbpo_trainer_f16_paths": (_i, [_p]),
    "cmbpo_trainer_fused": (_i, [_p]),
})

class TrainExtrasStruct(C.Structure):
    """ctypes image of ``cmbpo_train_extras_t``: sample weights [N], old predictions [N][D] (device pointers, NULL = off)
    and the clip range of the clipped value loss."""
    _fields_ = [("d_weights", C.c_void_p), ("d_old_pred", C.c_void_p), ("kl_cliprange", C.c_float)]


_ep = C.POINTER(TrainExtrasStruct)
SIGNATURES.update({
    "cmbpo_trainer_step_ex": (_i, [_p, _p, _i, _p, _i, _p, _i, _i, _ep, _p]),
    "cmbpo_trainer_epoch_ex": (_i, [_p, _p, _i, _p, _i, _p, _i, _i, _i, _ep, _p]),
    "cmbpo_trainer_losses_ex": (_i, [_p, _p, _i, _p, _i, _p, _i, _i, _p, _ep, _p]),
    "cmbpo_trainer_set_column_weights": (_i, [_p, _p, _p, _i, _p]),
    "cmbpo_trainer_set_column_kinds": (_i, [_p, _p, _i, _p]),
})

# start states of an imagined-rollout round (csrc/start_states.hip)
START_MAX_RUNS = 1024                          # CMBPO_START_MAX_RUNS
START_TABLE_INTS = 8 + 11 * START_MAX_RUNS     # CMBPO_START_TABLE_INTS
START_CDF_DOUBLES = 8 + 4 * START_MAX_RUNS     # CMBPO_START_CDF_DOUBLES
SIGNATURES.update({
    "cmbpo_start_table_build": (_i, [_p, C.c_long, _p, _p]),
    "cmbpo_start_epoch_draw": (_i, [_p, _p, _i, _i, _p, _p, _p, _p, C.c_long, _i, _i, _p, _p, _p, _p, _p]),
    "cmbpo_start_kl_parts": (_i, [_i]),
    "cmbpo_start_kl_partials": (_i, [_p] * 4 + [_i] * 3 + [_p, _i, _p]),
    "cmbpo_start_cdf": (_i, [_p, _p, _i, _i, _p, C.c_double, _p, _p]),
    "cmbpo_start_boltz_draw": (_i, [_p, _p, _p, _i, _p, C.c_long, _i, _p, _p, _p]),
})

# open-loop model validation: k-step replay of real trajectories (csrc/replay.hip)
REPLAY_OPEN_LOOP, REPLAY_ONE_STEP = 0, 1       # CMBPO_REPLAY_OPEN_LOOP / _ONE_STEP
REPLAY_SCALAR_SUMS, REPLAY_COUNTS = 4, 10      # columns of `sums` behind the obs_dim squared errors; columns of `counts`


class ReplayStruct(C.Structure):
    """ctypes image of ``cmbpo_replay_t`` (184 bytes), field for field."""
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "obs_dim", "act_dim", "mode", "reserved")] + \
               [(n, C.c_void_p) for n in ("act", "next_obs", "rew", "cost", "term", "len", "cur_obs", "alive",
                                          "p_next_obs", "p_rew", "p_term", "p_cost", "p_dkl_path", "p_ep_var_mean",
                                          "mean", "var", "part_sum", "part_cnt", "sums", "counts")]


_pp = C.POINTER(ReplayStruct)
SIGNATURES.update({
    "cmbpo_replay_parts": (_i, [_i]),
    "cmbpo_replay_compare": (_i, [_pp, _i, _p]),
    "cmbpo_replay_finish": (_i, [_pp, _p]),
    "cmbpo_replay_run": (_i, [_pp, _p, _i, _i, _p, _p]),
})

# predictive calibration in the replay: per calibrated column (obs_dim + 1 of them) six float64 sums and four int64 counts
REPLAY_CALIB_SUMS, REPLAY_CALIB_COUNTS = 6, 4  # CMBPO_REPLAY_CALIB_SUMS / _COUNTS


class ReplayCalibStruct(C.Structure):
    """ctypes image of ``cmbpo_replay_calib_t`` (56 bytes), field for field."""
    _fields_ = [(n, C.c_int32) for n in ("ensemble", "out_dim", "reserved")] + \
               [(n, C.c_void_p) for n in ("elite", "part_sum", "part_cnt", "sums", "counts")]


_cpp = C.POINTER(ReplayCalibStruct)
SIGNATURES.update({
    "cmbpo_replay_calibrate": (_i, [_pp, _cpp, _i, _p]),
    "cmbpo_replay_calib_finish": (_i, [_pp, _cpp, _p]),
    "cmbpo_replay_run_calibrated": (_i, [_pp, _cpp, _p, _i, _i, _p]),
})

# ... with the learned termination head in its post step
SIGNATURES.update({
    "cmbpo_replay_run_term": (_i, [_pp, _cpp, _tp, _p, _i, _i, _p, _p]),
})

# ... and with the cost head's reading (the superset)
SIGNATURES.update({
    "cmbpo_replay_run_cost": (_i, [_pp, _cpp, _tp, _chp, _p, _i, _i, _p, _p]),
})

# reliability tables of the logistic columns in the replay: per (column, reading) 2 K + 2 float64 sums and 2 K int64 counts
RELIAB_COST, RELIAB_TERM = 0, 1                                   # CMBPO_RELIAB_COST / _TERM: the recorded flag of a column
RELIAB_MAX_BINS, RELIAB_MAX_COLS, RELIAB_MAX_ENSEMBLE = 32, 2, 8  # CMBPO_RELIAB_MAX_*
RELIAB_TARGETS = {"cost": RELIAB_COST, "term": RELIAB_TERM}


class ReplayReliabStruct(C.Structure):
    """ctypes image of ``cmbpo_replay_reliab_t`` (104 bytes), field for field."""
    _fields_ = [(n, C.c_int32) for n in ("ensemble", "out_dim", "n_bins", "n_cols", "reserved")] + \
               [("col", C.c_int32 * 2), ("target", C.c_int32 * 2), ("shift", C.c_float * 2)] + \
               [(n, C.c_void_p) for n in ("elite", "edges", "term", "part_sum", "part_cnt", "sums", "counts")]


_rrp = C.POINTER(ReplayReliabStruct)
SIGNATURES.update({
    "cmbpo_replay_reliab": (_i, [_pp, _rrp, _i, _p]),
    "cmbpo_replay_reliab_finish": (_i, [_pp, _rrp, _p]),
    "cmbpo_replay_run_reliab": (_i, [_pp, _cpp, _rrp, _tp, _chp, _p, _i, _i, _p, _p]),
})

# the static rules' votes in the replay: a histogram of the two vote counts against the recorded flags, int64 only
REPLAY_VOTE_COUNTS, REPLAY_VOTES_MAX_ENSEMBLE = 38, 8             # CMBPO_REPLAY_VOTE_COUNTS / _VOTES_MAX_ENSEMBLE
REPLAY_VOTE_SLOTS = REPLAY_VOTES_MAX_ENSEMBLE + 1                 # v = 0 .. 8: counts = hist_cost [9][2] | hist_term [9][2] | n_vote | n_skipped


class ReplayVotesStruct(C.Structure):
    """ctypes image of ``cmbpo_replay_votes_t`` (56 bytes), field for field."""
    _fields_ = [(n, C.c_int32) for n in ("ensemble", "done_members", "cost_members", "reserved")] + \
               [(n, C.c_void_p) for n in ("done_votes", "cost_votes", "term", "part_cnt", "counts")]


_rvtp = C.POINTER(ReplayVotesStruct)
SIGNATURES.update({
    "cmbpo_replay_votes": (_i, [_pp, _rvtp, _i, _p]),
    "cmbpo_replay_votes_finish": (_i, [_pp, _rvtp, _p]),
    "cmbpo_replay_run_votes": (_i, [_pp, _cpp, _rrp, _rvtp, _tp, _chp, _p, _i, _i, _p, _p]),
})

# particle replay: a window's S sampled particles against the recording -- rank histograms, CRPS terms, moments
REPLAY_PARTICLES_MAX_OBS = 384                                    # CMBPO_REPLAY_PARTICLES_MAX_OBS
REPLAY_PARTICLES_MAX = 64                                         # S: a power of two in 2..64


class ReplayParticlesStruct(C.Structure):
    """ctypes image of ``cmbpo_replay_particles_t`` (200 bytes), field for field."""
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "S", "obs_dim", "act_dim", "mode", "reserved", "reserved2")] + \
               [(n, C.c_void_p) for n in ("act", "next_obs", "rew", "cost", "term", "len", "xi", "cur_obs", "alive",
                                          "p_next_obs", "p_rew", "p_term", "p_cost", "p_dkl_path", "p_ep_var_mean",
                                          "mean", "var", "part_sum", "part_cnt", "sums", "counts")]


_rpp = C.POINTER(ReplayParticlesStruct)
SIGNATURES.update({
    "cmbpo_replay_particles_parts": (_i, [_i, _i]),
    "cmbpo_replay_particles": (_i, [_rpp, _i, _p]),
    "cmbpo_replay_particles_finish": (_i, [_rpp, _p]),
    "cmbpo_replay_run_particles": (_i, [_rpp, _tp, _chp, _p, _i, _i, _p, _p]),
})

_lib = None


class CmbpoHipError(RuntimeError):
    pass


def lib():
    """Load (once) and return the ctypes handle; raise if the HIP library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CmbpoHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # torch first: its wheel bundles its own libamdhip64 / libhsa-runtime64, and the library must bind to THAT
        # runtime (the one that owns the tensors it is handed).  Loaded the other way round the process ends up with
        # two HIP runtimes and the second one finds no device.
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().cmbpo_last_error().decode("utf-8", "replace")
        raise CmbpoHipError(f"{what} failed (rc={rc}): {msg}")


def ptr(t):
    """Device (or host) pointer of a torch tensor / numpy array, None -> NULL."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data


def current_stream():
    """Raw hipStream_t of torch's current stream on the current device (the C call behind
    ``torch.cuda.current_stream().cuda_stream``, which costs ~8 us of Python per call -- it is asked for before every
    kernel launch, seven times per rollout step)."""
    import torch
    try:
        return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())
    except AttributeError:      # other torch builds: the public, slower route
        return torch.cuda.current_stream().cuda_stream

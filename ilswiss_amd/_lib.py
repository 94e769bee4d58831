"""ctypes binding of libilsx.so (include/ilsx.h).  No CPU fallback: importing the product path without
the built HIP library raises, and creating a context without an MI355X raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libilsx.so")

c_f32p = C.POINTER(C.c_float)
c_u8p = C.POINTER(C.c_uint8)
c_i64p = C.POINTER(C.c_int64)
vp = C.c_void_p


class MlpCfg(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32),
                ("out_dim", C.c_int32), ("n_heads", C.c_int32), ("act", C.c_int32), ("hidden_sizes", C.c_int32 * 3)]


class SacCfg(C.Structure):
    _fields_ = [("reward_scale", C.c_float), ("discount", C.c_float), ("policy_lr", C.c_float),
                ("qf_lr", C.c_float), ("alpha_lr", C.c_float), ("soft_target_tau", C.c_float),
                ("alpha", C.c_float), ("train_alpha", C.c_int32),
                ("policy_mean_reg_weight", C.c_float), ("policy_std_reg_weight", C.c_float),
                ("beta_1", C.c_float), ("has_target_entropy", C.c_int32), ("target_entropy", C.c_float),
                ("max_batch", C.c_int32), ("grad_world", C.c_int32)]


class SacStats(C.Structure):
    _fields_ = [("qf1_loss", C.c_float), ("qf2_loss", C.c_float), ("policy_loss", C.c_float),
                ("alpha_loss", C.c_float), ("alpha", C.c_float), ("q1_mean", C.c_float),
                ("q2_mean", C.c_float), ("log_pi_mean", C.c_float), ("policy_mu_mean", C.c_float),
                ("policy_log_std_mean", C.c_float), ("log_alpha", C.c_double),
                ("ext_std", C.c_float * 5), ("ext_max", C.c_float * 5), ("ext_min", C.c_float * 5)]


_MB, _MG = 8, 8


class PlanarModel(C.Structure):  # ilsx_planar_model
    _fields_ = [("task", C.c_int32), ("n_body", C.c_int32), ("n_geom", C.c_int32), ("frame_skip", C.c_int32),
                ("pgs_iters", C.c_int32), ("pad0", C.c_int32),
                ("parent", C.c_int32 * _MB), ("limited", C.c_int32 * _MB), ("geom_body", C.c_int32 * _MG),
                ("anchor", (C.c_double * 2) * _MB), ("com", (C.c_double * 2) * _MB),
                ("mass", C.c_double * _MB), ("inertia", C.c_double * _MB), ("jsign", C.c_double * _MB),
                ("armature", C.c_double * _MB), ("damping", C.c_double * _MB), ("range", (C.c_double * 2) * _MB),
                ("gear", C.c_double * _MB),
                ("geom_p1", (C.c_double * 2) * _MG), ("geom_p2", (C.c_double * 2) * _MG),
                ("geom_radius", C.c_double * _MG), ("geom_friction", C.c_double * _MG),
                ("timestep", C.c_double), ("gravity", C.c_double), ("reset_noise", C.c_double),
                ("contact_margin", C.c_double), ("contact_solref", C.c_double * 2), ("contact_solimp", C.c_double * 3),
                ("limit_solref", C.c_double * 2), ("limit_solimp", C.c_double * 3),
                ("ctrl_cost", C.c_double), ("alive_bonus", C.c_double), ("z_min", C.c_double), ("z_max", C.c_double),
                ("ang_max", C.c_double), ("state_max", C.c_double), ("init_qpos", C.c_double * (_MB + 2)),
                ("stiffness", C.c_double * _MB), ("reset_noise_vel_std", C.c_double), ("qvel_clip", C.c_double),
                ("max_rows", C.c_int32), ("pad1", C.c_int32)]


_ML3, _MC3, _MB3 = 20, 32, 16


_MC = 3    # ILSX_CARTCHAIN_MAX_DOF


class CartChainModel(C.Structure):  # ilsx_cartchain_model
    _fields_ = [("n_pole", C.c_int32), ("frame_skip", C.c_int32), ("pgs_iters", C.c_int32), ("limited", C.c_int32 * _MC),
                ("mass", C.c_double * _MC), ("inertia", C.c_double * _MC), ("com", (C.c_double * 2) * _MC), ("anchor", (C.c_double * 2) * _MC),
                ("armature", C.c_double * _MC), ("damping", C.c_double * _MC), ("range", (C.c_double * 2) * _MC),
                ("tip", C.c_double * 2), ("gear", C.c_double), ("ctrl_range", C.c_double * 2), ("jsign", C.c_double),
                ("timestep", C.c_double), ("gravity", C.c_double), ("limit_solref", C.c_double * 2), ("limit_solimp", C.c_double * 3)]


_MSL = 4            # ILSX_SWIMMER_MAX_LINK
_MSD = _MSL + 2     # ILSX_SWIMMER_MAX_DOF


class SwimmerModel(C.Structure):  # ilsx_swimmer_model
    _fields_ = [("n_link", C.c_int32), ("frame_skip", C.c_int32), ("pgs_iters", C.c_int32), ("limited", C.c_int32 * _MSD),
                ("mass", C.c_double * _MSL), ("inertia", (C.c_double * 3) * _MSL), ("box", (C.c_double * 3) * _MSL),
                ("com", (C.c_double * 2) * _MSL), ("anchor", (C.c_double * 2) * _MSL),
                ("armature", C.c_double * _MSD), ("damping", C.c_double * _MSD), ("range", (C.c_double * 2) * _MSD),
                ("gear", C.c_double * _MSD), ("init_qpos", C.c_double * _MSD),
                ("ctrl_range", C.c_double * 2), ("timestep", C.c_double), ("density", C.c_double), ("viscosity", C.c_double),
                ("limit_solref", C.c_double * 2), ("limit_solimp", C.c_double * 3)]


class LunarModel(C.Structure):  # ilsx_lunar_model
    _fields_ = [("frame_skip", C.c_int32), ("pgs_iters", C.c_int32),
                ("fps", C.c_double), ("scale", C.c_double), ("w", C.c_double), ("h", C.c_double), ("gravity", C.c_double),
                ("main_engine_power", C.c_double), ("side_engine_power", C.c_double), ("initial_random", C.c_double),
                ("side_engine_height", C.c_double), ("side_engine_away", C.c_double), ("leg_down", C.c_double), ("helipad_y", C.c_double),
                ("mass", C.c_double), ("inertia", C.c_double), ("com", C.c_double * 2), ("foot", (C.c_double * 2) * 2),
                ("hull", (C.c_double * 2) * 6),
                ("friction", C.c_double), ("contact_solref", C.c_double * 2), ("contact_solimp", C.c_double * 3),
                ("sleep_lin_tol", C.c_double), ("sleep_ang_tol", C.c_double), ("sleep_time", C.c_double)]


class GoalModel(C.Structure):  # ilsx_goal_model
    _fields_ = [("tol", C.c_double), ("step_scale", C.c_double), ("p_range", C.c_double), ("g_range", C.c_double),
                ("reward_kind", C.c_int32), ("pad", C.c_int32)]


class SpatialModel(C.Structure):  # ilsx_spatial_model
    _fields_ = [("task", C.c_int32), ("n_link", C.c_int32), ("n_act", C.c_int32), ("n_contact", C.c_int32),
                ("n_body", C.c_int32), ("frame_skip", C.c_int32), ("pgs_iters", C.c_int32), ("max_rows", C.c_int32),
                ("parent", C.c_int32 * _ML3), ("limited", C.c_int32 * _ML3), ("act_link", C.c_int32 * _ML3),
                ("contact_link", C.c_int32 * _MC3), ("body_link", C.c_int32 * _MB3),
                ("anchor", (C.c_double * 3) * _ML3), ("axis", (C.c_double * 3) * _ML3), ("quat0", (C.c_double * 4) * _ML3),
                ("com", (C.c_double * 3) * _ML3), ("mass", C.c_double * _ML3), ("inertia", (C.c_double * 6) * _ML3),
                ("armature", C.c_double * _ML3), ("damping", C.c_double * _ML3), ("stiffness", C.c_double * _ML3),
                ("range", (C.c_double * 2) * _ML3), ("gear", C.c_double * _ML3),
                ("contact_pos", (C.c_double * 3) * _MC3), ("contact_radius", C.c_double * _MC3),
                ("contact_friction", C.c_double * _MC3),
                ("timestep", C.c_double), ("gravity", C.c_double), ("reset_noise", C.c_double),
                ("reset_noise_vel_std", C.c_double), ("contact_margin", C.c_double), ("ctrl_range", C.c_double),
                ("contact_solref", C.c_double * 2), ("contact_solimp", C.c_double * 3),
                ("limit_solref", C.c_double * 2), ("limit_solimp", C.c_double * 3),
                ("ctrl_cost", C.c_double), ("alive_bonus", C.c_double), ("vel_weight", C.c_double), ("z_min", C.c_double),
                ("z_max", C.c_double), ("init_qpos", C.c_double * (_ML3 + 6)),
                ("obs_trunc", C.c_int32), ("pad0", C.c_int32)]


class Td3Cfg(C.Structure):  # ilsx_td3_cfg
    _fields_ = [("reward_scale", C.c_float), ("discount", C.c_float), ("policy_lr", C.c_float), ("qf_lr", C.c_float),
                ("policy_and_target_update_period", C.c_int32), ("soft_target_tau", C.c_float),
                ("policy_noise", C.c_float), ("policy_noise_clip", C.c_float), ("max_act", C.c_float),
                ("max_batch", C.c_int32), ("her", C.c_int32), ("clip_return_l", C.c_float), ("clip_return_r", C.c_float)]


class Td3Stats(C.Structure):  # ilsx_td3_stats
    _fields_ = [("qf1_loss", C.c_float), ("qf2_loss", C.c_float), ("policy_loss", C.c_float),
                ("q1_pred", C.c_float * 4), ("q2_pred", C.c_float * 4), ("q_target", C.c_float * 4),
                ("bellman1", C.c_float * 4), ("bellman2", C.c_float * 4), ("policy_action", C.c_float * 4)]


class DdpgCfg(C.Structure):  # ilsx_ddpg_cfg
    _fields_ = [("discount", C.c_float), ("policy_lr", C.c_float), ("qf_lr", C.c_float), ("qf_weight_decay", C.c_float),
                ("soft_target_tau", C.c_float), ("use_soft_update", C.c_int32), ("target_update_period", C.c_int32),
                ("policy_pre_activation_weight", C.c_float), ("min_q_value", C.c_float), ("max_q_value", C.c_float),
                ("max_act", C.c_float), ("max_batch", C.c_int32)]


class DdpgStats(C.Structure):  # ilsx_ddpg_stats
    _fields_ = [("qf_loss", C.c_float), ("policy_loss", C.c_float), ("raw_policy_loss", C.c_float),
                ("preactivation_policy_loss", C.c_float), ("q_pred", C.c_float * 4), ("q_target", C.c_float * 4),
                ("bellman", C.c_float * 4), ("policy_action", C.c_float * 4)]


class ExploreCfg(C.Structure):  # ilsx_explore_cfg
    _fields_ = [("kind", C.c_int32), ("pad", C.c_int32), ("mu", C.c_double), ("theta", C.c_double), ("max_sigma", C.c_double),
                ("min_sigma", C.c_double), ("decay_period", C.c_double), ("low", C.c_double), ("high", C.c_double)]


class DsacCfg(C.Structure):  # ilsx_dsac_cfg
    _fields_ = [("discount", C.c_float), ("reward_scale", C.c_float), ("alpha", C.c_float), ("soft_target_tau", C.c_float),
                ("policy_lr", C.c_float), ("qf_lr", C.c_float), ("beta_1", C.c_float), ("max_batch", C.c_int32)]


class DsacStats(C.Structure):  # ilsx_dsac_stats
    _fields_ = [("qf1_loss", C.c_float), ("qf2_loss", C.c_float), ("policy_loss", C.c_float),
                ("q1_pred", C.c_float * 4), ("q2_pred", C.c_float * 4)]


class DqnCfg(C.Structure):  # ilsx_dqn_cfg
    _fields_ = [("discount", C.c_float), ("learning_rate", C.c_float), ("tau", C.c_float), ("use_hard_updates", C.c_int32),
                ("hard_update_period", C.c_int32), ("double_q", C.c_int32), ("max_batch", C.c_int32)]


class DqnStats(C.Structure):  # ilsx_dqn_stats
    _fields_ = [("qf_loss", C.c_float), ("y_pred", C.c_float * 4)]


class SacvCfg(C.Structure):  # ilsx_sacv_cfg
    _fields_ = [("reward_scale", C.c_float), ("discount", C.c_float), ("alpha", C.c_float), ("policy_lr", C.c_float),
                ("qf_lr", C.c_float), ("vf_lr", C.c_float), ("soft_target_tau", C.c_float),
                ("policy_mean_reg_weight", C.c_float), ("policy_std_reg_weight", C.c_float), ("beta_1", C.c_float),
                ("max_batch", C.c_int32)]


class SacvStats(C.Structure):  # ilsx_sacv_stats
    _fields_ = [("qf1_loss", C.c_float), ("qf2_loss", C.c_float), ("vf_loss", C.c_float), ("policy_loss", C.c_float),
                ("q1_pred", C.c_float * 4), ("q2_pred", C.c_float * 4), ("v_pred", C.c_float * 4),
                ("log_pi", C.c_float * 4), ("policy_mu", C.c_float * 4), ("policy_log_std", C.c_float * 4)]


class BcCfg(C.Structure):  # ilsx_bc_cfg
    _fields_ = [("mode", C.c_int32), ("lr", C.c_float), ("momentum", C.c_float), ("max_batch", C.c_int32)]


class GcslCfg(C.Structure):  # ilsx_gcsl_cfg
    _fields_ = [("mode", C.c_int32), ("policy_lr", C.c_float), ("max_batch", C.c_int32), ("d_obs", C.c_int32), ("d_goal", C.c_int32),
                ("horizon", C.c_int32)]


class PpoCfg(C.Structure):  # ilsx_ppo_cfg
    _fields_ = [("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("n_hidden", C.c_int32), ("hidden", C.c_int32),
                ("reward_scale", C.c_float), ("discount", C.c_float), ("clip_eps", C.c_float),
                ("policy_lr", C.c_float), ("value_lr", C.c_float), ("gae_tau", C.c_float),
                ("value_l2_reg", C.c_float), ("mini_batch_size", C.c_int32), ("update_epoch", C.c_int32),
                ("max_samples", C.c_int32), ("use_value_clip", C.c_int32), ("conditioned_std", C.c_int32),
                ("hidden_sizes", C.c_int32 * 3), ("grad_world", C.c_int32)]


class DiscCfg(C.Structure):  # ilsx_disc_cfg
    _fields_ = [("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("hid_dim", C.c_int32), ("hid_act", C.c_int32),
                ("use_grad_pen", C.c_int32), ("clamp_magnitude", C.c_float), ("disc_lr", C.c_float),
                ("disc_momentum", C.c_float), ("grad_pen_weight", C.c_float), ("max_batch", C.c_int32),
                ("state_only", C.c_int32), ("num_layer_blocks", C.c_int32), ("use_bn", C.c_int32), ("grad_world", C.c_int32)]


class OptMeta(C.Structure):  # ilsx_opt_meta
    _fields_ = [("t", C.c_int64), ("rng_step", C.c_uint64), ("n_train_steps", C.c_int64)]


class BnnCfg(C.Structure):  # ilsx_bnn_cfg
    _fields_ = [("ensemble", C.c_int32), ("in_dim", C.c_int32), ("out_dim", C.c_int32), ("hidden", C.c_int32), ("n_hidden", C.c_int32),
                ("max_batch", C.c_int32), ("lr", C.c_float), ("reward_scale", C.c_float), ("init_w", C.c_float),
                ("weight_decay", C.c_float * 9)]


class DiscStats(C.Structure):
    _fields_ = [("ce_loss", C.c_float), ("grad_pen", C.c_float), ("accuracy", C.c_float)]


# name -> (restype, argtypes); every symbol include/ilsx.h declares
PROTOTYPES = {
    "ilsx_sac_group_create": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.POINTER(vp)]),
    "ilsx_sac_group_destroy": (C.c_int, [vp]),
    "ilsx_sac_group_train_from_replay": (C.c_int, [vp, C.POINTER(vp), C.c_int, C.c_int, C.c_int]),
    "ilsx_advirl_train": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                    C.c_int, C.c_float, C.POINTER(DiscStats), C.POINTER(SacStats), vp]),
    "ilsx_net_set_noise_policy": (C.c_int, [vp, C.c_float, C.c_float, C.c_float]),
    "ilsx_net_set_output_linear": (C.c_int, [vp, C.c_int]),
    "ilsx_td3_create": (C.c_int, [vp, C.POINTER(Td3Cfg), vp, vp, vp, C.POINTER(vp)]),
    "ilsx_td3_destroy": (C.c_int, [vp]),
    "ilsx_td3_train_step": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(Td3Stats)]),
    "ilsx_td3_train_from_replay": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(Td3Stats)]),
    "ilsx_td3_get_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_td3_set_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_ddpg_create": (C.c_int, [vp, C.POINTER(DdpgCfg), vp, vp, C.POINTER(vp)]),
    "ilsx_ddpg_destroy": (C.c_int, [vp]),
    "ilsx_ddpg_train_step": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(DdpgStats)]),
    "ilsx_ddpg_train_from_replay": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(DdpgStats)]),
    "ilsx_ddpg_get_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_ddpg_set_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_ddpg_get_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_ddpg_set_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_vecenv_set_exploration": (C.c_int, [vp, C.POINTER(ExploreCfg)]),
    "ilsx_vecenv_set_exploration_t": (C.c_int, [vp, C.c_int64]),
    "ilsx_vecenv_explore": (C.c_int, [vp, vp, vp, C.c_int64]),
    "ilsx_vecenv_set_exploration_epsilon": (C.c_int, [vp, C.c_double]),
    "ilsx_vecenv_explore_u": (C.c_int, [vp, vp, vp, vp, C.c_int64]),
    "ilsx_sacv_create": (C.c_int, [vp, C.POINTER(SacvCfg), vp, vp, vp, vp, C.POINTER(vp)]),
    "ilsx_sacv_destroy": (C.c_int, [vp]),
    "ilsx_sacv_train_step": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(SacvStats)]),
    "ilsx_sacv_train_from_replay": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(SacvStats)]),
    "ilsx_sacv_get_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_sacv_set_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_bc_create": (C.c_int, [vp, C.POINTER(BcCfg), vp, C.POINTER(vp)]),
    "ilsx_bc_destroy": (C.c_int, [vp]),
    "ilsx_bc_train_step": (C.c_int, [vp, vp, vp, C.c_int, vp, C.POINTER(C.c_float)]),
    "ilsx_bc_train_from_replay": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "ilsx_ppo_create": (C.c_int, [vp, C.POINTER(PpoCfg), C.POINTER(vp)]),
    "ilsx_ppo_destroy": (C.c_int, [vp]),
    "ilsx_ppo_num_params": (C.c_int, [vp, C.c_int, C.POINTER(C.c_size_t)]),
    "ilsx_ppo_set_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_ppo_get_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_ppo_gae": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp]),
    "ilsx_ppo_values": (C.c_int, [vp, vp, C.c_int, vp]),
    "ilsx_ppo_train": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, vp]),
    "ilsx_rollout_step_relabel": (C.c_int, [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int]),
    "ilsx_eval_rollout": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp]),
    "ilsx_ppo_rollout": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]),
    "ilsx_vecenv_set_obs_affine": (C.c_int, [vp, vp, vp]),
    "ilsx_is_terminal": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, vp]),
    "ilsx_vecenv_obs_norm": (C.c_int, [vp, C.c_int, C.c_int]),
    "ilsx_vecenv_get_obs_rms": (C.c_int, [vp, vp, vp, C.POINTER(C.c_double)]),
    "ilsx_vecenv_set_obs_rms": (C.c_int, [vp, vp, vp, C.c_double]),
    "ilsx_ppo_debug_perm": (C.c_int, [vp, C.c_int, C.c_uint32, vp]),
    "ilsx_ppo_debug_grad_norm": (C.c_int, [vp, C.POINTER(C.c_float)]),
    "ilsx_ppo_policy_act": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp]),
    "ilsx_disc_create": (C.c_int, [vp, C.POINTER(DiscCfg), C.POINTER(vp)]),
    "ilsx_advirl_set_policy_batch_from_expert": (C.c_int, [vp, C.c_int]),
    "ilsx_her_gather": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp, vp]),
    "ilsx_her_sample": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp, vp, vp, vp, vp]),
    "ilsx_debug_rng_stream": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    "ilsx_debug_philox": (C.c_int, [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_int, vp, vp]),
    "ilsx_debug_ctx_allocs": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
    "ilsx_disc_destroy": (C.c_int, [vp]),
    "ilsx_disc_num_params": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
    "ilsx_disc_set_params": (C.c_int, [vp, vp, C.c_size_t]),
    "ilsx_disc_get_params": (C.c_int, [vp, vp, C.c_size_t]),
    "ilsx_disc_get_grads": (C.c_int, [vp, vp, C.c_size_t]),
    "ilsx_disc_get_bn_stats": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "ilsx_disc_set_bn_stats": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "ilsx_disc_train_step": (C.c_int, [vp, vp, vp, vp, vp, C.c_int, vp, C.POINTER(DiscStats)]),
    "ilsx_disc_reward": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, vp, vp]),
    "ilsx_vecenv_create": (C.c_int, [vp, C.POINTER(PlanarModel), C.c_int, C.c_uint64, C.POINTER(vp)]),
    "ilsx_vecenv_create_spatial": (C.c_int, [vp, C.POINTER(SpatialModel), C.c_int, C.c_uint64, C.POINTER(vp)]),
    "ilsx_vecenv_state_dims": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ilsx_vecenv_set_path_mode": (C.c_int, [vp, C.c_int]),
    "ilsx_vecenv_destroy": (C.c_int, [vp]),
    "ilsx_vecenv_dims": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ilsx_vecenv_reset": (C.c_int, [vp, vp, C.c_int, vp]),
    "ilsx_vecenv_step": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, vp]),
    "ilsx_vecenv_get_state": (C.c_int, [vp, vp, vp]),
    "ilsx_vecenv_set_state": (C.c_int, [vp, vp, vp]),
    "ilsx_vecenv_cur_obs": (C.c_int, [vp, C.POINTER(vp)]),
    "ilsx_rollout_step": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ilsx_rollout_step_begin": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "ilsx_rollout_step_end": (C.c_int, [vp]),
    "ilsx_eval_rollouts_lockstep": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_double)]),
    "ilsx_rollout_steps_lockstep": (C.c_int, [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int, C.c_int]),
    "ilsx_rollout_stats": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int]),
    "ilsx_abi_version": (C.c_int, []),
    "ilsx_last_error": (C.c_char_p, []),
    "ilsx_ctx_create": (C.c_int, [C.c_int, vp, C.c_uint64, C.POINTER(vp)]),
    "ilsx_ctx_sync": (C.c_int, [vp]),
    "ilsx_ctx_destroy": (C.c_int, [vp]),
    "ilsx_ctx_stream": (vp, [vp]),
    "ilsx_ctx_rng_stream_cursor": (C.c_int, [vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    "ilsx_ctx_alloc": (C.c_int, [vp, C.c_size_t, C.POINTER(vp)]),
    "ilsx_ctx_free": (C.c_int, [vp, vp]),
    "ilsx_memcpy_h2d": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "ilsx_memcpy_d2h": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "ilsx_comm_unique_id": (C.c_int, [vp]),
    "ilsx_comm_init": (C.c_int, [vp, vp, C.c_int, C.c_int]),
    "ilsx_comm_destroy": (C.c_int, [vp]),
    "ilsx_comm_info": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ilsx_comm_allreduce_sum": (C.c_int, [vp, vp, C.c_size_t]),
    "ilsx_td3_get_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_td3_set_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_sacv_get_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_sacv_set_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_bc_get_opt": (C.c_int, [vp, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_bc_set_opt": (C.c_int, [vp, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_ppo_get_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_ppo_set_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_disc_get_opt": (C.c_int, [vp, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_disc_set_opt": (C.c_int, [vp, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_prof_enable": (C.c_int, [vp, C.c_int]),
    "ilsx_prof_reset": (C.c_int, [vp]),
    "ilsx_prof_read": (C.c_int, [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    "ilsx_prof_kernel": (C.c_char_p, [vp, C.c_int]),
    "ilsx_kernel_name": (C.c_char_p, [C.c_int]),
    "ilsx_debug_set_stamp_buffer": (C.c_int, [vp, vp, C.c_int, C.POINTER(C.c_int)]),
    "ilsx_debug_dw_split": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ilsx_net_create": (C.c_int, [vp, C.POINTER(MlpCfg), C.POINTER(vp)]),
    "ilsx_net_destroy": (C.c_int, [vp]),
    "ilsx_net_num_params": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
    "ilsx_net_init": (C.c_int, [vp, C.c_uint64, C.c_float, C.c_float]),
    "ilsx_net_set_params": (C.c_int, [vp, vp, C.c_size_t, C.c_int]),
    "ilsx_net_get_params": (C.c_int, [vp, vp, C.c_size_t, C.c_int]),
    "ilsx_mlp_forward": (C.c_int, [vp, vp, C.c_int, vp]),
    "ilsx_policy_act": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, vp]),
    "ilsx_policy_log_prob": (C.c_int, [vp, vp, vp, C.c_int, vp]),
    "ilsx_replay_create": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_uint64, C.POINTER(vp)]),
    "ilsx_replay_destroy": (C.c_int, [vp]),
    "ilsx_replay_add": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int]),
    "ilsx_replay_terminate_episode": (C.c_int, [vp]),
    "ilsx_replay_set_absorbing": (C.c_int, [vp, C.c_int64, C.c_int, vp]),
    "ilsx_replay_get_absorbing": (C.c_int, [vp, vp, C.c_int, vp]),
    "ilsx_replay_sample": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]),
    "ilsx_replay_sample_many": (C.c_int, [vp, C.c_int, C.c_int, vp]),
    "ilsx_replay_record_floats": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "ilsx_replay_size": (C.c_int, [vp, c_i64p, c_i64p]),
    "ilsx_replay_clear": (C.c_int, [vp]),
    "ilsx_replay_traj_endpoints": (C.c_int, [vp, c_i64p, c_i64p, C.c_int, C.POINTER(C.c_int)]),
    "ilsx_sac_create": (C.c_int, [vp, C.POINTER(SacCfg), vp, vp, vp, C.POINTER(vp)]),
    "ilsx_sac_destroy": (C.c_int, [vp]),
    "ilsx_sac_train_step": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.POINTER(SacStats)]),
    "ilsx_sac_train_from_replay": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(SacStats)]),
    "ilsx_sac_set_batch": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, vp, vp]),
    "ilsx_sac_critic_backward": (C.c_int, [vp]),
    "ilsx_sac_critic_update": (C.c_int, [vp]),
    "ilsx_sac_actor_backward": (C.c_int, [vp]),
    "ilsx_sac_actor_update": (C.c_int, [vp]),
    "ilsx_sac_last_stats": (C.c_int, [vp, C.POINTER(SacStats)]),
    "ilsx_sac_get_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t, C.c_int]),
    "ilsx_sac_set_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t, C.c_int]),
    "ilsx_sac_get_grads": (C.c_int, [vp, C.c_int, vp, C.c_size_t, C.c_int]),
    "ilsx_sac_grads_ptr": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]),
    "ilsx_sac_get_log_alpha": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "ilsx_sac_set_log_alpha": (C.c_int, [vp, C.c_double]),
    "ilsx_sac_get_adam": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, c_i64p]),
    "ilsx_sac_set_adam": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.c_int64]),
    "ilsx_sac_get_alpha_opt": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), c_i64p, C.POINTER(C.c_uint64)]),
    "ilsx_sac_debug_batch": (C.c_int, [vp, vp, C.c_uint64, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "ilsx_sac_debug_last_batch": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, vp]),
    "ilsx_sac_phase_state": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ilsx_sac_debug_break_phase": (C.c_int, [vp]),
    "ilsx_debug_phase_static_ok": (C.c_int, [C.c_int] * 10),
    "ilsx_sac_set_alpha_opt": (C.c_int, [vp, C.c_double, C.c_double, C.c_int64, C.c_uint64]),
    "ilsx_bnn_create": (C.c_int, [vp, C.POINTER(BnnCfg), C.POINTER(vp)]),
    "ilsx_bnn_destroy": (C.c_int, [vp]),
    "ilsx_bnn_num_params": (C.c_int, [vp, C.POINTER(C.c_size_t)]),
    "ilsx_bnn_init": (C.c_int, [vp, C.c_uint64]),
    "ilsx_bnn_get_params": (C.c_int, [vp, vp, C.c_size_t]),
    "ilsx_bnn_set_params": (C.c_int, [vp, vp, C.c_size_t]),
    "ilsx_bnn_get_opt": (C.c_int, [vp, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_bnn_set_opt": (C.c_int, [vp, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_bnn_set_normalizer": (C.c_int, [vp, vp, vp]),
    "ilsx_bnn_get_normalizer": (C.c_int, [vp, vp, vp]),
    "ilsx_bnn_fit_stats": (C.c_int, [vp, vp, vp, C.c_int]),
    "ilsx_bnn_train_batch": (C.c_int, [vp, vp, vp, C.c_int64, C.c_int, vp]),
    "ilsx_bnn_mse": (C.c_int, [vp, vp, vp, C.c_int64, C.c_int, C.c_int, vp]),
    "ilsx_bnn_predict": (C.c_int, [vp, vp, C.c_int, vp, vp, C.c_int]),
    "ilsx_bnn_debug_padding": (C.c_int, [vp, C.POINTER(C.c_double)]),
    "ilsx_net_set_categorical": (C.c_int, [vp, C.c_int]),
    "ilsx_policy_log_pis": (C.c_int, [vp, vp, C.c_int, vp]),
    "ilsx_vecenv_create_classic": (C.c_int, [vp, C.c_int, C.c_int, C.c_uint64, C.POINTER(vp)]),
    "ilsx_vecenv_create_cartchain": (C.c_int, [vp, C.POINTER(CartChainModel), C.c_int, C.c_uint64, C.POINTER(vp)]),
    "ilsx_vecenv_create_swimmer": (C.c_int, [vp, C.POINTER(SwimmerModel), C.c_int, C.c_uint64, C.POINTER(vp)]),
    "ilsx_vecenv_create_lunar": (C.c_int, [vp, C.POINTER(LunarModel), C.c_int, C.c_uint64, C.POINTER(vp)]),
    "ilsx_vecenv_create_goal": (C.c_int, [vp, C.POINTER(GoalModel), C.c_int, C.c_uint64, C.POINTER(vp)]),
    "ilsx_vecenv_goal_dims": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "ilsx_vecenv_action_space": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "ilsx_dsac_create": (C.c_int, [vp, C.POINTER(DsacCfg), vp, vp, vp, C.POINTER(vp)]),
    "ilsx_dsac_destroy": (C.c_int, [vp]),
    "ilsx_dsac_train_step": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(DsacStats)]),
    "ilsx_dsac_train_from_replay": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(DsacStats)]),
    "ilsx_dsac_get_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_dsac_set_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_dsac_get_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_dsac_set_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_net_set_epsilon_greedy": (C.c_int, [vp, C.c_int, C.c_float]),
    "ilsx_dqn_create": (C.c_int, [vp, C.POINTER(DqnCfg), vp, C.POINTER(vp)]),
    "ilsx_dqn_destroy": (C.c_int, [vp]),
    "ilsx_dqn_train_step": (C.c_int, [vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(DqnStats)]),
    "ilsx_dqn_train_from_replay": (C.c_int, [vp, vp, C.c_int, C.c_int, C.POINTER(DqnStats)]),
    "ilsx_dqn_get_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_dqn_set_params": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_dqn_get_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_dqn_set_opt": (C.c_int, [vp, C.c_int, vp, vp, C.c_size_t, C.POINTER(OptMeta)]),
    "ilsx_mbpo_model_step": (C.c_int, [vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp,
                                       C.POINTER(C.c_int)]),
    "ilsx_her_horizon_gather": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]),
    "ilsx_bncat_create": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "ilsx_bncat_destroy": (C.c_int, [vp]),
    "ilsx_bncat_num_params": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "ilsx_bncat_get": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_bncat_set": (C.c_int, [vp, C.c_int, vp, C.c_size_t]),
    "ilsx_bncat_get_meta": (C.c_int, [vp, C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]),
    "ilsx_bncat_set_meta": (C.c_int, [vp, C.c_int64, C.c_uint64]),
    "ilsx_bncat_input": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
    "ilsx_bncat_train_step": (C.c_int, [vp, C.c_int, C.c_float, vp]),
    "ilsx_bncat_act": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp]),
    "ilsx_gcsl_create": (C.c_int, [vp, C.POINTER(GcslCfg), vp, vp, C.c_int, C.POINTER(vp)]),
    "ilsx_gcsl_destroy": (C.c_int, [vp]),
    "ilsx_gcsl_train_from_replay": (C.c_int, [vp, vp, vp, vp, C.c_int, vp]),
    "ilsx_gcsl_train_step": (C.c_int, [vp, vp, vp, C.c_int, vp]),
}

_lib = None


def load():
    """Load libilsx.so (once).  Raises RuntimeError if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("ILSX_LIB", LIB_PATH)   # ILSX_LIB: a measurement build of the same library (libilsx_stamps.so), never a fallback
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C ilswiss_amd/csrc`.  ilswiss_amd has no CPU fallback.")
    lib = C.CDLL(path)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here == header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if lib.ilsx_abi_version() != 1:
        raise RuntimeError(f"libilsx ABI {lib.ilsx_abi_version()} != 1")
    _lib = lib
    return lib


ILSX_ERR_UNSUPPORTED = -5   # include/ilsx.h


def check(rc):
    if rc != 0:
        msg = load().ilsx_last_error()
        raise RuntimeError(f"libilsx error {rc}: {msg.decode() if msg else '?'}")

"""ctypes bindings of include/cordic_amd.h (no arithmetic lives here)."""
import ctypes as C
import os

P2R, R2P, SP2R, SR2P = 0, 1, 2, 3
MAX_STAGES = 64
FLAG_FORCE_GENERIC = 0x1
FLAG_NO_LJ = 0x4
FLAG_NO_SEED = 0x8
FLAG_STATIC_CHUNKS = 0x20
FLAG_UNIT_GAIN = 0x10
FLAG_NO_TAILS = 0x40
# enum cordic_status (the codes tests assert on)
ERR_MODE = -1
ERR_UNSUPPORTED = -6
ERR_ARGS, ERR_DEVICE, ERR_CONTAINER = -7, -8, -9

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    # CORDIC_AMD_LIB: an alternative build of the same library (A/B work)
    return os.environ.get("CORDIC_AMD_LIB",
                          os.path.join(_HERE, "libcordic_amd.so"))


class CordicError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        msg = lib().cordic_strerror(status).decode()
        super().__init__("%s: %s (status %d)" % (what, msg, status))


class _CConfig(C.Structure):
    _fields_ = [
        ("mode", C.c_int32), ("iw", C.c_int32), ("ow", C.c_int32),
        ("nextra", C.c_int32), ("ww", C.c_int32), ("pw", C.c_int32),
        ("nstages", C.c_int32), ("clocks_per_output", C.c_int32),
        ("quantization_variance", C.c_double),
        ("phase_variance_rad", C.c_double),
        ("gain", C.c_double), ("best_possible_cnr", C.c_double),
        ("has_reset", C.c_int32), ("has_aux", C.c_int32),
        ("async_reset", C.c_int32),
        ("nlive", C.c_int32), ("needs_wrap", C.c_int32),
        ("flags", C.c_uint32),
        ("angle", C.c_uint32 * MAX_STAGES),
    ]


_lib = None

_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)
_cfgp = C.POINTER(_CConfig)

# name -> (restype, argtypes): every symbol include/cordic_amd.h declares
ABI = {
    "cordic_abi_version": (C.c_int, []),
    "cordic_strerror": (C.c_char_p, [C.c_int]),
    "cordic_config_init": (C.c_int, [_cfgp] + [C.c_int] * 6),
    "cordic_config_init_core": (C.c_int, [_cfgp] + [C.c_int] * 6),
    "cordic_config_from_args": (C.c_int, [_cfgp, C.c_int,
                                          C.POINTER(C.c_char_p), C.c_char_p,
                                          C.c_size_t, C.POINTER(C.c_int)]),
    "cordic_config_write_header": (C.c_int, [_cfgp, C.c_char_p, C.c_char_p,
                                             C.c_size_t]),
    "cordic_nextlg": (C.c_int, [C.c_uint]),
    "cordic_gain": (C.c_double, [C.c_int]),
    "cordic_phase_variance": (C.c_double, [C.c_int, C.c_int]),
    "cordic_transform_quantization_variance": (C.c_double, [C.c_int] * 3),
    "cordic_angles": (C.c_int, [C.c_int, C.c_int, _u32p]),
    "cordic_calc_stages_ww": (C.c_int, [C.c_int, C.c_int]),
    "cordic_calc_stages": (C.c_int, [C.c_int]),
    "cordic_calc_phase_bits": (C.c_int, [C.c_int]),
    "cordic_p2r": (C.c_int, [_cfgp, C.c_size_t, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_p2r_const": (C.c_int, [_cfgp, C.c_size_t, C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "cordic_nco": (C.c_int, [_cfgp, C.c_size_t, C.c_uint32, C.c_uint32,
                             C.c_uint64, C.c_int32, C.c_int32, C.c_void_p,
                             C.c_void_p, C.c_void_p]),
    "cordic_r2p": (C.c_int, [_cfgp, C.c_size_t, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_p2r16": (C.c_int, [_cfgp, C.c_size_t, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "cordic_p2r16_const": (C.c_int, [_cfgp, C.c_size_t, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "cordic_nco16": (C.c_int, [_cfgp, C.c_size_t, C.c_uint32, C.c_uint32,
                               C.c_uint64, C.c_int32, C.c_int32, C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    "cordic_r2p16": (C.c_int, [_cfgp, C.c_size_t, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_plan_p2r16_const": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32,
                                          C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "cordic_plan_nco16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                    C.c_uint32, C.c_uint64, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "cordic_mix16": (C.c_int, [_cfgp, C.c_size_t, C.c_uint32, C.c_uint32,
                               C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]),
    "cordic_plan_mix16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                    C.c_uint32, C.c_uint64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    "cordic_plan_p2r16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "cordic_jobset_create16": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t,
                                         C.c_void_p, C.POINTER(C.c_void_p)]),
    "cordic_plan_create": (C.c_int, [_cfgp, C.POINTER(C.c_void_p)]),
    "cordic_plan_destroy": (None, [C.c_void_p]),
    "cordic_plan_config": (_cfgp, [C.c_void_p]),
    "cordic_plan_seed_info": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p]),
    "cordic_plan_p2r_const": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int32,
                                        C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "cordic_plan_nco": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                  C.c_uint32, C.c_uint64, C.c_int32,
                                  C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "cordic_seed_table": (C.c_size_t, [_cfgp, _u32p, C.c_size_t]),
    "cordic_dir_table": (C.c_size_t, [_cfgp, _u32p, C.c_size_t]),
    "cordic_plan_tail_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]),
    "cordic_plan_queue_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_plan_prepare": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_void_p]),
    "cordic_host_set_devices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
    "cordic_host_lane_stats": (C.c_int, [C.c_int, C.c_void_p]),
    "cordic_mix": (C.c_int, [_cfgp, C.c_size_t, C.c_uint32, C.c_uint32,
                             C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p]),
    "cordic_plan_mix": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                  C.c_uint32, C.c_uint64, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "cordic_jobset_create": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t,
                                       C.c_void_p, C.POINTER(C.c_void_p)]),
    "cordic_jobset_destroy": (None, [C.c_void_p]),
    "cordic_jobset_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32)]),
    "cordic_jobset_path": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "cordic_plan_run_jobs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_void_p]),
    "cordic_plan_p2r_const_batch": (C.c_int, [C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_int32, C.c_int32,
                                              C.c_void_p]),
    "cordic_plan_nco_batch": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_int32, C.c_int32, C.c_void_p]),
    "cordic_plan_r2p_batch": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p]),
    "cordic_plan_p2r_batch": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p]),
    "cordic_plan_mix_batch": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p]),
    "cordic_jobset_reap": (None, []),
    "cordic_plan_image_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]),
    "cordic_plan_set_min_samples": (C.c_int, [C.c_void_p, C.c_longlong]),
    "cordic_plan_p2r": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "cordic_plan_dir_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32)]),
    "cordic_table_queue_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_quad_queue_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_device_count": (C.c_int, []),
    "cordic_shard_range": (C.c_int, [C.c_uint64, C.c_int, C.c_int,
                                     C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64)]),
    "cordic_group_create": (C.c_int, [_cfgp, C.c_int, C.POINTER(C.c_int),
                                      C.c_int, C.c_int,
                                      C.POINTER(C.c_void_p)]),
    "cordic_group_destroy": (None, [C.c_void_p]),
    "cordic_group_size": (C.c_int, [C.c_void_p]),
    "cordic_group_range": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int,
                                     C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64)]),
    "cordic_group_reserve": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int]),
    "cordic_group_set_placement": (C.c_int, [C.c_void_p, C.c_int]),
    "cordic_arrays_alloc": (C.c_int, [C.c_size_t, C.c_int, C.c_int,
                                      C.POINTER(C.c_void_p), C.c_void_p]),
    "cordic_arrays_free": (None, [C.POINTER(C.c_void_p), C.c_int]),
    "cordic_group_placement": (C.c_int, [C.c_void_p, C.c_int,
                                         C.POINTER(C.c_int), C.POINTER(C.c_int)]
                               + [C.POINTER(C.c_float)] * 4),
    "cordic_group_fill_phase_ramp": (C.c_int, [C.c_void_p, C.c_uint64,
                                               C.c_int]),
    "cordic_group_fill_iq_ramp": (C.c_int, [C.c_void_p, C.c_uint64,
                                            C.c_uint32, C.c_uint32, C.c_int]),
    "cordic_group_p2r_const": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int32,
                                         C.c_int32]),
    "cordic_group_nco": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32,
                                   C.c_uint32, C.c_int32, C.c_int32]),
    "cordic_group_r2p": (C.c_int, [C.c_void_p, C.c_uint64]),
    "cordic_group_sync": (C.c_int, [C.c_void_p]),
    "cordic_group_digest": (C.c_int, [C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64)]),
    "cordic_group_set_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_int]),
    "cordic_rccl_unique_id": (C.c_int, [C.c_void_p]),
    "cordic_group_rccl_init": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_group_set_gather_rccl": (C.c_int, [C.c_void_p, C.c_int,
                                               C.c_void_p, C.c_void_p,
                                               C.c_int]),
    "cordic_group_mark": (C.c_int, [C.c_void_p, C.c_int]),
    "cordic_group_elapsed": (C.c_int, [C.c_void_p, C.c_int, C.c_int,
                                       C.POINTER(C.c_float),
                                       C.POINTER(C.c_float)]),
    "cordic_group_buffers": (C.c_int, [C.c_void_p, C.c_int,
                                       C.POINTER(C.c_int)] +
                             [C.POINTER(C.c_void_p)] * 4 +
                             [C.POINTER(C.c_uint64)]),
    "cordic_group_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_uint64,
                                    C.c_uint64, C.c_void_p]),
    "cordic_group_write": (C.c_int, [C.c_void_p, C.c_int, C.c_int,
                                     C.c_uint64, C.c_uint64, C.c_void_p]),
    "cordic_gain_annihilator": (C.c_uint32, [C.c_int]),
    "cordic_config_gain_annihilator": (C.c_uint32, [_cfgp]),
    "cordic_stream_create": (C.c_int, [_cfgp, C.POINTER(C.c_void_p)]),
    "cordic_stream_destroy": (None, [C.c_void_p]),
    "cordic_stream_workspace": (C.c_size_t, [C.c_size_t]),
    "cordic_stream_reserve": (C.c_int, [C.c_void_p, C.c_size_t]),
    "cordic_stream_latency": (C.c_int, [C.c_void_p]),
    "cordic_stream_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_stream_ticks": (C.c_int, [C.c_void_p, C.c_size_t] +
                            [C.c_void_p] * 10),
    "cordic_table_lds_mode": (C.c_int, [C.c_void_p]),
    "cordic_seq_create": (C.c_int, [_cfgp, C.POINTER(C.c_void_p)]),
    "cordic_seq_destroy": (None, [C.c_void_p]),
    "cordic_seq_workspace": (C.c_size_t, [C.c_size_t]),
    "cordic_seq_reserve": (C.c_int, [C.c_void_p, C.c_size_t]),
    "cordic_seq_ticks": (C.c_int, [C.c_void_p, C.c_size_t] +
                         [C.c_void_p] * 12),
    "cordic_seq_violations": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cordic_quad_config_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int,
                                          C.c_int, C.c_int]),
    "cordic_quad_config_init_core": (C.c_int, [C.c_void_p, C.c_int, C.c_int,
                                               C.c_int]),
    "cordic_quad_tables": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p,
                                     C.c_size_t]),
    "cordic_quad_write_header": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p,
                                           C.c_size_t]),
    "cordic_quad_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "cordic_quad_destroy": (None, [C.c_void_p]),
    "cordic_quad_lookup": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "cordic_quad_nco": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                   C.c_uint32, C.c_uint64, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "cordic_quad_nco16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                   C.c_uint32, C.c_uint64, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "cordic_table_config_init": (C.c_int, [C.c_void_p] + [C.c_int] * 4),
    "cordic_table_values": (C.c_int, [C.c_void_p, _i32p, C.c_size_t]),
    "cordic_table_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "cordic_table_destroy": (None, [C.c_void_p]),
    "cordic_table_lookup": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "cordic_table_nco": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                   C.c_uint32, C.c_uint64, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "cordic_table_nco16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                   C.c_uint32, C.c_uint64, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "cordic_fm_workspace": (C.c_size_t, [C.c_size_t]),
    "cordic_phase_accumulate": (C.c_int, [C.c_size_t, C.c_void_p, C.c_void_p,
                                          C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "cordic_table_fm": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_void_p, C.c_uint32, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "cordic_table_fm16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "cordic_quad_fm": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "cordic_quad_fm16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "cordic_fm_demod_workspace": (C.c_size_t, [C.c_size_t]),
    "cordic_fm_demod_info": (C.c_int, [_cfgp, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32)]),
    "cordic_fm_demod": (C.c_int, [_cfgp, C.c_size_t, C.c_void_p, C.c_void_p,
                                  C.c_uint32, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_fm_demod16": (C.c_int, [_cfgp, C.c_size_t, C.c_void_p, C.c_void_p,
                                    C.c_uint32, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_fm_demod16_info": (C.c_int, [_cfgp, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32)]),
    "cordic_demodbank_create": (C.c_int, [_cfgp, C.c_size_t, C.c_void_p,
                                          C.POINTER(C.c_void_p)]),
    "cordic_demodbank_create16": (C.c_int, [_cfgp, C.c_size_t, C.c_void_p,
                                            C.POINTER(C.c_void_p)]),
    "cordic_demodbank_destroy": (None, [C.c_void_p]),
    "cordic_demodbank_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]),
    "cordic_demodbank_run": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_plan_fm_mix_workspace": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "cordic_plan_fm_mix_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32)]),
    "cordic_plan_fm_mix": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_plan_fm_mix16_workspace": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "cordic_plan_fm_mix16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_plan_fm_mix_decim_workspace": (C.c_size_t, [C.c_void_p, C.c_size_t,
                                                        C.c_uint32]),
    "cordic_plan_fm_mix_decim": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "cordic_plan_fm_mix_decim16_workspace": (C.c_size_t, [C.c_void_p,
                                                          C.c_size_t,
                                                          C.c_uint32]),
    "cordic_plan_fm_mix_decim16": (C.c_int, [C.c_void_p, C.c_size_t,
                                             C.c_uint32, C.c_void_p,
                                             C.c_void_p, C.c_uint32,
                                             C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "cordic_mixbank_create_decim": (C.c_int, [C.c_void_p, C.c_uint32,
                                              C.c_size_t, C.c_void_p,
                                              C.POINTER(C.c_void_p)]),
    "cordic_mixbank_create_decim16": (C.c_int, [C.c_void_p, C.c_uint32,
                                                C.c_size_t, C.c_void_p,
                                                C.POINTER(C.c_void_p)]),
    "cordic_mixbank_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.POINTER(C.c_void_p)]),
    "cordic_mixbank_create16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.POINTER(C.c_void_p)]),
    "cordic_plan_fm_mix_c16_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32)]),
    "cordic_plan_fm_mix_c16_workspace": (C.c_size_t, [C.c_void_p, C.c_size_t]),
    "cordic_plan_fm_mix_c16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                         C.c_void_p, C.c_uint32, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "cordic_plan_fm_mix_decim_c16_workspace": (C.c_size_t, [C.c_void_p,
                                                            C.c_size_t,
                                                            C.c_uint32]),
    "cordic_plan_fm_mix_decim_c16": (C.c_int, [C.c_void_p, C.c_size_t,
                                               C.c_uint32, C.c_void_p,
                                               C.c_void_p, C.c_uint32,
                                               C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    "cordic_mixbank_create_c16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.POINTER(C.c_void_p)]),
    "cordic_mixbank_create_decim_c16": (C.c_int, [C.c_void_p, C.c_uint32,
                                                  C.c_size_t, C.c_void_p,
                                                  C.POINTER(C.c_void_p)]),
    "cordic_mixbank_destroy": (None, [C.c_void_p]),
    "cordic_mixbank_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32)]),
    "cordic_mixbank_run": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_plan_fm_rx_workspace": (C.c_size_t, [C.c_void_p, _cfgp, C.c_size_t]),
    "cordic_plan_fm_rx16_workspace": (C.c_size_t, [C.c_void_p, _cfgp,
                                                   C.c_size_t]),
    "cordic_plan_fm_rx_info": (C.c_int, [C.c_void_p, _cfgp,
                                         C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32)]),
    "cordic_plan_fm_rx16_info": (C.c_int, [C.c_void_p, _cfgp,
                                           C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32)]),
    "cordic_plan_fm_rx": (C.c_int, [C.c_void_p, _cfgp, C.c_size_t, C.c_void_p,
                                    C.c_void_p, C.c_uint32, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "cordic_plan_fm_rx16": (C.c_int, [C.c_void_p, _cfgp, C.c_size_t,
                                      C.c_void_p, C.c_void_p, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_plan_fm_rx_decim_workspace": (C.c_size_t, [C.c_void_p, _cfgp,
                                                       C.c_size_t, C.c_uint32]),
    "cordic_plan_fm_rx_decim16_workspace": (C.c_size_t, [C.c_void_p, _cfgp,
                                                         C.c_size_t,
                                                         C.c_uint32]),
    "cordic_plan_fm_rx_decim": (C.c_int, [C.c_void_p, _cfgp, C.c_size_t,
                                          C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_uint32, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "cordic_plan_fm_rx_decim16": (C.c_int, [C.c_void_p, _cfgp, C.c_size_t,
                                            C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_uint32, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_uint32, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "cordic_rxbank_create": (C.c_int, [C.c_void_p, _cfgp, C.c_size_t,
                                       C.c_void_p, C.POINTER(C.c_void_p)]),
    "cordic_rxbank_create16": (C.c_int, [C.c_void_p, _cfgp, C.c_size_t,
                                         C.c_void_p, C.POINTER(C.c_void_p)]),
    "cordic_rxbank_create_decim": (C.c_int, [C.c_void_p, _cfgp, C.c_uint32,
                                             C.c_size_t, C.c_void_p,
                                             C.POINTER(C.c_void_p)]),
    "cordic_rxbank_create_decim16": (C.c_int, [C.c_void_p, _cfgp, C.c_uint32,
                                               C.c_size_t, C.c_void_p,
                                               C.POINTER(C.c_void_p)]),
    "cordic_plan_fm_rx_c16_workspace": (C.c_size_t, [C.c_void_p, _cfgp,
                                                     C.c_size_t]),
    "cordic_plan_fm_rx_c16_info": (C.c_int, [C.c_void_p, _cfgp,
                                             C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32)]),
    "cordic_plan_fm_rx_c16": (C.c_int, [C.c_void_p, _cfgp, C.c_size_t,
                                        C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "cordic_plan_fm_rx_decim_c16_workspace": (C.c_size_t, [C.c_void_p, _cfgp,
                                                           C.c_size_t,
                                                           C.c_uint32]),
    "cordic_plan_fm_rx_decim_c16": (C.c_int, [C.c_void_p, _cfgp, C.c_size_t,
                                              C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_uint32,
                                              C.c_void_p, C.c_void_p,
                                              C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "cordic_rxbank_create_c16": (C.c_int, [C.c_void_p, _cfgp, C.c_size_t,
                                           C.c_void_p, C.POINTER(C.c_void_p)]),
    "cordic_rxbank_create_decim_c16": (C.c_int, [C.c_void_p, _cfgp, C.c_uint32,
                                                 C.c_size_t, C.c_void_p,
                                                 C.POINTER(C.c_void_p)]),
    "cordic_rxbank_destroy": (None, [C.c_void_p]),
    "cordic_rxbank_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32)]),
    "cordic_rxbank_run": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_table_bank_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.POINTER(C.c_void_p)]),
    "cordic_table_bank_create16": (C.c_int, [C.c_void_p, C.c_size_t,
                                             C.c_void_p,
                                             C.POINTER(C.c_void_p)]),
    "cordic_quad_bank_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.POINTER(C.c_void_p)]),
    "cordic_quad_bank_create16": (C.c_int, [C.c_void_p, C.c_size_t,
                                            C.c_void_p,
                                            C.POINTER(C.c_void_p)]),
    "cordic_oscbank_destroy": (None, [C.c_void_p]),
    "cordic_oscbank_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64),
                                      C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32)]),
    "cordic_oscbank_run": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p]),
    "cordic_oscbank_retune": (C.c_int, [C.c_void_p, C.c_size_t, C.c_size_t,
                                        C.c_void_p, C.c_void_p]),
    "cordic_table_fmbank_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.POINTER(C.c_void_p)]),
    "cordic_table_fmbank_create16": (C.c_int, [C.c_void_p, C.c_size_t,
                                               C.c_void_p,
                                               C.POINTER(C.c_void_p)]),
    "cordic_quad_fmbank_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                            C.POINTER(C.c_void_p)]),
    "cordic_quad_fmbank_create16": (C.c_int, [C.c_void_p, C.c_size_t,
                                              C.c_void_p,
                                              C.POINTER(C.c_void_p)]),
    "cordic_fmbank_destroy": (None, [C.c_void_p]),
    "cordic_fmbank_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_int32)]),
    "cordic_fmbank_run": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_p2r_host": (C.c_int, [_cfgp, C.c_size_t, _i32p, _i32p, C.c_int,
                                  _u32p, _i32p, _i32p]),
    "cordic_host_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t]),
    "cordic_host_free": (None, [C.c_void_p]),
    "cordic_host_release": (None, []),
    "cordic_host_last_stats": (C.c_int, [C.c_void_p]),
    "cordic_r2p_host": (C.c_int, [_cfgp, C.c_size_t, _i32p, _i32p, _i32p,
                                  _u32p]),
    "cordic_fill_phase_ramp": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64,
                                         C.c_int, C.c_void_p]),
    "cordic_fill_iq_ramp": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.c_int, C.c_void_p]),
    "cordic_digest_u32": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64,
                                    C.c_void_p, C.c_void_p]),
    "cordic_last_kernel": (C.c_int, []),
    "cordic_quality_create": (C.c_int, [_cfgp, C.POINTER(C.c_void_p)]),
    "cordic_quality_destroy": (None, [C.c_void_p]),
    "cordic_quality_reset": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_quality_p2r": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "cordic_quality_nco": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                     C.c_uint32, C.c_uint64, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "cordic_quality_r2p": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "cordic_quality_p2r_result": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_quality_r2p_result": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_quality_create_quad": (C.c_int, [C.c_void_p,
                                             C.POINTER(C.c_void_p)]),
    "cordic_quality_create_table": (C.c_int, [C.c_void_p,
                                              C.POINTER(C.c_void_p)]),
    "cordic_quality_sine": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "cordic_quality_sine16": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "cordic_quality_sine_nco": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint32,
                                          C.c_uint32, C.c_uint64, C.c_void_p,
                                          C.c_void_p]),
    "cordic_quality_sine_nco16": (C.c_int, [C.c_void_p, C.c_size_t,
                                            C.c_uint32, C.c_uint32,
                                            C.c_uint64, C.c_void_p,
                                            C.c_void_p]),
    "cordic_quality_sine_result": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cordic_sfdr_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "cordic_sfdr_destroy": (None, [C.c_void_p]),
    "cordic_sfdr_load_iq": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_sfdr_load_sine": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64,
                                        C.c_void_p, C.c_void_p]),
    "cordic_sfdr_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cordic_sfdr_bins": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64,
                                   C.c_void_p]),
    "cordic_fill_circle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t,
                                     C.c_uint64, C.c_int, C.c_int, C.c_int,
                                     C.c_void_p]),
}


def lib():
    """Load libcordic_amd.so; raise (never fall back) if it is absent."""
    global _lib
    if _lib is None:
        # PyTorch-ROCm ships its own libamdhip64; whichever copy is loaded
        # first serves the whole process.  Tensors handed to this library are
        # allocated by torch, so torch's runtime must be the one in use: load
        # it before libcordic_amd.so pulls in /opt/rocm's copy (two runtimes
        # in one process make every launch fail).  Pure C++ callers never see
        # this file and simply use the system runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = lib_path()
        if not os.path.exists(path):
            raise ImportError(
                "%s not built: run `python -c 'import __graft_entry__ as g; "
                "g.build()'` (there is no CPU fallback)" % path)
        L = C.CDLL(path)
        for name, (res, args) in ABI.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise CordicError(rc, what)


class Config:
    """One generated core (cordic_config)."""

    def __init__(self, c):
        self.c = c

    @classmethod
    def from_cli(cls, mode, iw=-1, ow=-1, xtra=2, pw=-1, nstages=-1):
        c = _CConfig()
        _check(lib().cordic_config_init(C.byref(c), mode, iw, ow, xtra, pw,
                                        nstages), "cordic_config_init")
        return cls(c)

    @classmethod
    def from_core(cls, mode, nstages, iw, ow, nxtra, pw):
        c = _CConfig()
        _check(lib().cordic_config_init_core(C.byref(c), mode, nstages, iw,
                                             ow, nxtra, pw),
               "cordic_config_init_core")
        return cls(c)

    @classmethod
    def from_args(cls, args):
        """args: gencordic command line without the program name."""
        if isinstance(args, str):
            args = args.split()
        argv = (C.c_char_p * (len(args) + 1))(
            b"gencordic", *[a.encode() for a in args])
        c = _CConfig()
        fname = C.create_string_buffer(512)
        hdr = C.c_int(0)
        _check(lib().cordic_config_from_args(C.byref(c), len(args) + 1, argv,
                                             fname, 512, C.byref(hdr)),
               "cordic_config_from_args")
        cfg = cls(c)
        cfg.fname = fname.value.decode()
        cfg.c_header = bool(hdr.value)
        return cfg

    def header_text(self, name):
        buf = C.create_string_buffer(4096)
        n = lib().cordic_config_write_header(C.byref(self.c), name.encode(),
                                             buf, 4096)
        if n < 0:
            raise CordicError(n, "cordic_config_write_header")
        return buf.value.decode()

    def __getattr__(self, k):
        return getattr(self.c, k)

    @property
    def angles(self):
        return list(self.c.angle[: self.c.nstages])

    def with_flags(self, flags):
        c = _CConfig()
        C.memmove(C.byref(c), C.byref(self.c), C.sizeof(_CConfig))
        c.flags = flags
        return Config(c)

    @property
    def ref(self):
        return C.byref(self.c)


class Plan:
    """cordic_plan: a generated core bound to the current device."""

    def __init__(self, cfg):
        self.cfg = cfg
        h = C.c_void_p()
        _check(lib().cordic_plan_create(cfg.ref, C.byref(h)),
               "cordic_plan_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib().cordic_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def seed_info(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().cordic_plan_seed_info(self._h, C.byref(a), C.byref(b),
                                           C.byref(c)),
               "cordic_plan_seed_info")
        return dict(stages=a.value, nleaves=b.value, nbuckets=c.value)

    @property
    def dir_groups(self):
        """stages per looked-up group of the per-sample-vector path
        (cordic_plan_p2r); [] = that feed runs cordic_p2r's kernel"""
        n = C.c_int32()
        st = (C.c_int32 * 5)()
        _check(lib().cordic_plan_dir_info(self._h, C.byref(n), st),
               "cordic_plan_dir_info")
        return [int(st[g]) for g in range(n.value)]

    def p2r(self, x, y, phase, ox, oy, n=None, stream=None):
        """per-sample vectors through the plan (directions looked up)"""
        n = phase.numel() if n is None else n
        if any(_is16(t) for t in (x, y, phase, ox, oy)):
            # (cordic_p2r16's kernel: no looked-up directions on int16 arrays)
            _same16("cordic_plan_p2r16", x, y, phase, ox, oy)
            _check(lib().cordic_plan_p2r16(
                self._h, n, _ptr(x), _ptr(y), _ptr(phase), _ptr(ox), _ptr(oy),
                _stream(stream)), "cordic_plan_p2r16")
            return
        _check(lib().cordic_plan_p2r(self._h, n, _ptr(x), _ptr(y), _ptr(phase),
                                     _ptr(ox), _ptr(oy), _stream(stream)),
               "cordic_plan_p2r")

    def mix(self, phase0, fcw, index0, x, y, ox, oy, n=None, stream=None):
        """fused NCO mixer through the plan (directions looked up)"""
        n = x.numel() if n is None else n
        if any(_is16(t) for t in (x, y, ox, oy)):
            _same16("cordic_plan_mix16", x, y, ox, oy)
            _check(lib().cordic_plan_mix16(
                self._h, n, phase0 & 0xffffffff, fcw & 0xffffffff, index0,
                _ptr(x), _ptr(y), _ptr(ox), _ptr(oy), _stream(stream)),
                "cordic_plan_mix16")
            return
        _check(lib().cordic_plan_mix(self._h, n, phase0 & 0xffffffff,
                                     fcw & 0xffffffff, index0, _ptr(x), _ptr(y),
                                     _ptr(ox), _ptr(oy), _stream(stream)),
               "cordic_plan_mix")

    def fm_mix_workspace(self, n):
        """cordic_plan_fm_mix_workspace: bytes of device scratch an fm_mix
        call of n samples needs on this plan (16-byte aligned)"""
        return int(lib().cordic_plan_fm_mix_workspace(self._h, n))

    def fm_mix_info(self):
        """cordic_plan_fm_mix_info: (fused, tile) -- whether fm_mix runs the
        fused kernel on this plan, and the samples a block makes per pass"""
        fused, tile = C.c_int32(0), C.c_int32(0)
        _check(lib().cordic_plan_fm_mix_info(self._h, C.byref(fused),
                                             C.byref(tile)),
               "cordic_plan_fm_mix_info")
        return int(fused.value), int(tile.value)

    def fm_mix(self, fcw, x, y, ox, oy, work=None, pm=None, n=None, phase0=0,
               acc=None, stream=None):
        """cordic_plan_fm_mix: (x, y) rotated by the running sum of the
        per-sample tuning words, phase[i] = phase0 + acc[0] + fcw[0] + .. +
        fcw[i-1] (+ pm[i]); acc (a one-word device tensor, optional) is left
        at the sum behind sample n-1.  work: device scratch of
        fm_mix_workspace(n) bytes (16-byte aligned), the caller's."""
        n = x.numel() if n is None else n
        _need_work(work, n, self.fm_mix_workspace, n)
        _check(lib().cordic_plan_fm_mix(
            self._h, n, _ptr(fcw), _ptr(pm), phase0 & 0xffffffff, _ptr(acc),
            _ptr(x), _ptr(y), _ptr(ox), _ptr(oy), _ptr(work), _stream(stream)),
            "cordic_plan_fm_mix")

    def fm_mix16_workspace(self, n):
        """cordic_plan_fm_mix16_workspace: bytes of device scratch an fm_mix16
        call of n samples needs on this plan (16-byte aligned)"""
        return int(lib().cordic_plan_fm_mix16_workspace(self._h, n))

    def fm_mix16(self, fcw, x, y, ox, oy, work=None, pm=None, n=None, phase0=0,
                 acc=None, stream=None):
        """cordic_plan_fm_mix16: fm_mix on int16 x, y, ox, oy (cores with IW
        and OW <= 16); fcw, pm and acc stay 32-bit words.  work: device
        scratch of fm_mix16_workspace(n) bytes (16-byte aligned), the
        caller's."""
        n = x.numel() if n is None else n
        _same16("cordic_plan_fm_mix16", x, y, ox, oy)
        _need_work(work, n, self.fm_mix16_workspace, n)
        _check(lib().cordic_plan_fm_mix16(
            self._h, n, _ptr(fcw), _ptr(pm), phase0 & 0xffffffff, _ptr(acc),
            _ptr(x), _ptr(y), _ptr(ox), _ptr(oy), _ptr(work), _stream(stream)),
            "cordic_plan_fm_mix16")

    def fm_mix_decim_workspace(self, n, log2r):
        """cordic_plan_fm_mix_decim_workspace: bytes of device scratch an
        fm_mix_decim call of n samples at R = 2**log2r needs on this plan
        (16-byte aligned); 0 where the call would fail"""
        return int(lib().cordic_plan_fm_mix_decim_workspace(self._h, n, log2r))

    def fm_mix_decim16_workspace(self, n, log2r):
        """cordic_plan_fm_mix_decim16_workspace: the same for fm_mix_decim16"""
        return int(lib().cordic_plan_fm_mix_decim16_workspace(self._h, n, log2r))

    def _fm_mix_decim(self, name, log2r, fcw, x, y, ox, oy, work, pm, n, phase0,
                      acc, stream):
        n = x.numel() if n is None else n
        _need_work(work, n, getattr(self, name + "_workspace"), n, log2r)
        cname = "cordic_plan_" + name
        _check(getattr(lib(), cname)(
            self._h, n, log2r, _ptr(fcw), _ptr(pm), phase0 & 0xffffffff,
            _ptr(acc), _ptr(x), _ptr(y), _ptr(ox), _ptr(oy), _ptr(work),
            _stream(stream)), cname)

    def fm_mix_decim(self, log2r, fcw, x, y, ox, oy, work=None, pm=None, n=None,
                     phase0=0, acc=None, stream=None):
        """cordic_plan_fm_mix_decim: fm_mix with an integrate-and-dump by R =
        2**log2r behind the rotator -- ox[j], oy[j] = floor(the sum of the R
        tuned samples jR .. jR + R - 1 / R), n >> log2r elements each; n a
        multiple of R, log2r in 0 .. 8 (0: fm_mix itself).  work: device
        scratch of fm_mix_decim_workspace(n, log2r) bytes, the caller's."""
        self._fm_mix_decim("fm_mix_decim", log2r, fcw, x, y, ox, oy, work, pm, n,
                           phase0, acc, stream)

    def fm_mix_decim16(self, log2r, fcw, x, y, ox, oy, work=None, pm=None,
                       n=None, phase0=0, acc=None, stream=None):
        """cordic_plan_fm_mix_decim16: fm_mix_decim on int16 x, y, ox, oy
        (cores with IW and OW <= 16); fcw, pm and acc stay 32-bit words."""
        _same16("cordic_plan_fm_mix_decim16", x, y, ox, oy)
        self._fm_mix_decim("fm_mix_decim16", log2r, fcw, x, y, ox, oy, work, pm,
                           n, phase0, acc, stream)

    def fm_mix_c16_info(self):
        """cordic_plan_fm_mix_c16_info: (fused, tile) of fm_mix_c16 on this
        plan -- fused where fm_mix16 is"""
        fused, tile = C.c_int32(0), C.c_int32(0)
        _check(lib().cordic_plan_fm_mix_c16_info(self._h, C.byref(fused),
                                                 C.byref(tile)),
               "cordic_plan_fm_mix_c16_info")
        return int(fused.value), int(tile.value)

    def fm_mix_c16_workspace(self, n):
        """cordic_plan_fm_mix_c16_workspace: bytes of device scratch an
        fm_mix_c16 call of n complex samples needs"""
        return int(lib().cordic_plan_fm_mix_c16_workspace(self._h, n))

    def fm_mix_decim_c16_workspace(self, n, log2r):
        """cordic_plan_fm_mix_decim_c16_workspace: the same for
        fm_mix_decim_c16 at R = 2**log2r; 0 where the call would fail"""
        return int(lib().cordic_plan_fm_mix_decim_c16_workspace(self._h, n,
                                                                log2r))

    def _fm_mix_c16(self, cname, wsize, args, fcw, iq, oiq, work, pm, n, phase0,
                    acc, stream):
        _same16(cname, iq, oiq)
        n = iq.numel() // 2 if n is None else n
        if hasattr(iq, "numel") and iq.numel() < 2 * n:
            raise ValueError("%s: iq holds %d shorts, 2 n = %d"
                             % (cname, iq.numel(), 2 * n))
        _need_work(work, n, wsize, n, *args)
        _check(getattr(lib(), cname)(
            self._h, n, *args, _ptr(fcw), _ptr(pm), phase0 & 0xffffffff,
            _ptr(acc), _ptr(iq), _ptr(oiq), _ptr(work), _stream(stream)), cname)

    def fm_mix_c16(self, fcw, iq, oiq, work=None, pm=None, n=None, phase0=0,
                   acc=None, stream=None):
        """cordic_plan_fm_mix_c16: fm_mix16 on INTERLEAVED int16 I/Q, in and
        out -- iq and oiq are int16 tensors of 2 n elements, I0 Q0 I1 Q1 ..
        The bits of fm_mix16 on iq[0::2], iq[1::2] in oiq[0::2], oiq[1::2].
        n None: iq.numel() // 2.  work: fm_mix_c16_workspace(n) bytes."""
        self._fm_mix_c16("cordic_plan_fm_mix_c16", self.fm_mix_c16_workspace,
                         (), fcw, iq, oiq, work, pm, n, phase0, acc, stream)

    def fm_mix_decim_c16(self, log2r, fcw, iq, oiq, work=None, pm=None, n=None,
                         phase0=0, acc=None, stream=None):
        """cordic_plan_fm_mix_decim_c16: fm_mix_decim16 on interleaved int16
        I/Q (iq: 2 n shorts); oiq holds 2 (n >> log2r) shorts.  work:
        fm_mix_decim_c16_workspace(n, log2r) bytes."""
        self._fm_mix_c16("cordic_plan_fm_mix_decim_c16",
                         self.fm_mix_decim_c16_workspace, (log2r,), fcw, iq,
                         oiq, work, pm, n, phase0, acc, stream)

    def fm_rx_workspace(self, conv, n):
        """cordic_plan_fm_rx_workspace: bytes of device scratch an fm_rx call
        of n samples into the converter `conv` needs (16-byte aligned)"""
        return int(lib().cordic_plan_fm_rx_workspace(
            self._h, conv.ref if conv is not None else None, n))

    def fm_rx16_workspace(self, conv, n):
        """cordic_plan_fm_rx16_workspace: the same for fm_rx16"""
        return int(lib().cordic_plan_fm_rx16_workspace(
            self._h, conv.ref if conv is not None else None, n))

    def _fm_rx_info(self, name, conv):
        fused, tile = C.c_int32(0), C.c_int32(0)
        _check(getattr(lib(), name)(
            self._h, conv.ref if conv is not None else None, C.byref(fused),
            C.byref(tile)), name)
        return int(fused.value), int(tile.value)

    def fm_rx_info(self, conv):
        """cordic_plan_fm_rx_info: (fused, tile) -- whether fm_rx into the
        converter `conv` runs the fused kernel, and the samples a block makes
        per pass"""
        return self._fm_rx_info("cordic_plan_fm_rx_info", conv)

    def fm_rx16_info(self, conv):
        """cordic_plan_fm_rx16_info: the same for fm_rx16"""
        return self._fm_rx_info("cordic_plan_fm_rx16_info", conv)

    def _fm_rx(self, name, wsize, conv, fcw, x, y, mag, freq, work, pm, n,
               phase0, acc, dphase0, last, stream):
        n = x.numel() if n is None else n
        _need_work(work, n, wsize, conv, n)
        _check(getattr(lib(), name)(
            self._h, conv.ref if conv is not None else None, n, _ptr(fcw),
            _ptr(pm), phase0 & 0xffffffff, _ptr(acc), _ptr(x), _ptr(y),
            dphase0 & 0xffffffff, _ptr(last), _ptr(mag), _ptr(freq),
            _ptr(work), _stream(stream)), name)

    def fm_rx(self, conv, fcw, x, y, mag, freq, work=None, pm=None, n=None,
              phase0=0, acc=None, dphase0=0, last=None, stream=None):
        """cordic_plan_fm_rx: fm_mix and fm_demod (on the r2p / sr2p core
        `conv`) in one call, the tuned I/Q never stored: mag and freq are what
        fm_demod gives on fm_mix's outputs.  acc and last (one-word device
        tensors, optional) carry the oscillator and the discriminator from
        call to call.  work: device scratch of fm_rx_workspace(conv, n) bytes
        (16-byte aligned), the caller's."""
        self._fm_rx("cordic_plan_fm_rx", self.fm_rx_workspace, conv, fcw, x, y,
                    mag, freq, work, pm, n, phase0, acc, dphase0, last, stream)

    def fm_rx16(self, conv, fcw, x, y, mag, freq, work=None, pm=None, n=None,
                phase0=0, acc=None, dphase0=0, last=None, stream=None):
        """cordic_plan_fm_rx16: fm_rx on int16 x, y, mag, freq (both cores
        within the 16-bit containers); fcw, pm, acc and last stay 32-bit
        words.  work: fm_rx16_workspace(conv, n) bytes."""
        _same16("cordic_plan_fm_rx16", x, y, mag, freq)
        self._fm_rx("cordic_plan_fm_rx16", self.fm_rx16_workspace, conv, fcw,
                    x, y, mag, freq, work, pm, n, phase0, acc, dphase0, last,
                    stream)

    def fm_rx_decim_workspace(self, conv, n, log2r):
        """cordic_plan_fm_rx_decim_workspace: bytes of device scratch an
        fm_rx_decim call of n samples at R = 2**log2r into the converter
        `conv` needs (16-byte aligned); 0 where the call would fail"""
        return int(lib().cordic_plan_fm_rx_decim_workspace(
            self._h, conv.ref if conv is not None else None, n, log2r))

    def fm_rx_decim16_workspace(self, conv, n, log2r):
        """cordic_plan_fm_rx_decim16_workspace: the same for fm_rx_decim16"""
        return int(lib().cordic_plan_fm_rx_decim16_workspace(
            self._h, conv.ref if conv is not None else None, n, log2r))

    def _fm_rx_decim(self, name, conv, log2r, fcw, x, y, mag, freq, work, pm,
                     n, phase0, acc, dphase0, last, stream):
        n = x.numel() if n is None else n
        _need_work(work, n, getattr(self, name + "_workspace"), conv, n, log2r)
        cname = "cordic_plan_" + name
        _check(getattr(lib(), cname)(
            self._h, conv.ref if conv is not None else None, n, log2r,
            _ptr(fcw), _ptr(pm), phase0 & 0xffffffff, _ptr(acc), _ptr(x),
            _ptr(y), dphase0 & 0xffffffff, _ptr(last), _ptr(mag), _ptr(freq),
            _ptr(work), _stream(stream)), cname)

    def fm_rx_decim(self, conv, log2r, fcw, x, y, mag, freq, work=None,
                    pm=None, n=None, phase0=0, acc=None, dphase0=0, last=None,
                    stream=None):
        """cordic_plan_fm_rx_decim: fm_mix_decim by R = 2**log2r and fm_demod
        (on the r2p / sr2p core `conv`) in one call, neither the tuned nor the
        decimated I/Q stored: mag and freq hold n >> log2r elements, what
        fm_demod gives on fm_mix_decim's outputs.  n a multiple of R, log2r in
        0 .. 8 (0: fm_rx itself).  work: device scratch of
        fm_rx_decim_workspace(conv, n, log2r) bytes, the caller's."""
        self._fm_rx_decim("fm_rx_decim", conv, log2r, fcw, x, y, mag, freq,
                          work, pm, n, phase0, acc, dphase0, last, stream)

    def fm_rx_decim16(self, conv, log2r, fcw, x, y, mag, freq, work=None,
                      pm=None, n=None, phase0=0, acc=None, dphase0=0,
                      last=None, stream=None):
        """cordic_plan_fm_rx_decim16: fm_rx_decim on int16 x, y, mag, freq
        (both cores within the 16-bit containers); fcw, pm, acc and last stay
        32-bit words."""
        _same16("cordic_plan_fm_rx_decim16", x, y, mag, freq)
        self._fm_rx_decim("fm_rx_decim16", conv, log2r, fcw, x, y, mag, freq,
                          work, pm, n, phase0, acc, dphase0, last, stream)

    def fm_rx_c16_workspace(self, conv, n):
        """cordic_plan_fm_rx_c16_workspace: bytes of device scratch an
        fm_rx_c16 call of n complex samples needs"""
        return int(lib().cordic_plan_fm_rx_c16_workspace(
            self._h, conv.ref if conv is not None else None, n))

    def fm_rx_c16_info(self, conv):
        """cordic_plan_fm_rx_c16_info: (fused, tile), fm_rx16_info's answer"""
        return self._fm_rx_info("cordic_plan_fm_rx_c16_info", conv)

    def fm_rx_decim_c16_workspace(self, conv, n, log2r):
        """cordic_plan_fm_rx_decim_c16_workspace: the same for
        fm_rx_decim_c16 at R = 2**log2r; 0 where the call would fail"""
        return int(lib().cordic_plan_fm_rx_decim_c16_workspace(
            self._h, conv.ref if conv is not None else None, n, log2r))

    def _fm_rx_c16(self, cname, wsize, args, conv, fcw, iq, mag, freq, work,
                   pm, n, phase0, acc, dphase0, last, stream):
        _same16(cname, iq, mag, freq)
        n = iq.numel() // 2 if n is None else n
        if hasattr(iq, "numel") and iq.numel() < 2 * n:
            raise ValueError("%s: iq holds %d shorts, 2 n = %d"
                             % (cname, iq.numel(), 2 * n))
        _need_work(work, n, wsize, conv, n, *args)
        _check(getattr(lib(), cname)(
            self._h, conv.ref if conv is not None else None, n, *args,
            _ptr(fcw), _ptr(pm), phase0 & 0xffffffff, _ptr(acc), _ptr(iq),
            dphase0 & 0xffffffff, _ptr(last), _ptr(mag), _ptr(freq),
            _ptr(work), _stream(stream)), cname)

    def fm_rx_c16(self, conv, fcw, iq, mag, freq, work=None, pm=None, n=None,
                  phase0=0, acc=None, dphase0=0, last=None, stream=None):
        """cordic_plan_fm_rx_c16: fm_rx16 on INTERLEAVED int16 I/Q -- iq is
        one int16 tensor of 2 n elements, I0 Q0 I1 Q1 .., as a capture
        delivers it; mag and freq are int16 tensors of n elements.  The bits
        of fm_rx16 on iq[0::2], iq[1::2].  n None: iq.numel() // 2.  work:
        fm_rx_c16_workspace(conv, n) bytes."""
        self._fm_rx_c16("cordic_plan_fm_rx_c16", self.fm_rx_c16_workspace, (),
                        conv, fcw, iq, mag, freq, work, pm, n, phase0, acc,
                        dphase0, last, stream)

    def fm_rx_decim_c16(self, conv, log2r, fcw, iq, mag, freq, work=None,
                        pm=None, n=None, phase0=0, acc=None, dphase0=0,
                        last=None, stream=None):
        """cordic_plan_fm_rx_decim_c16: fm_rx_decim16 on interleaved int16
        I/Q (iq: 2 n shorts); mag and freq hold n >> log2r shorts.  work:
        fm_rx_decim_c16_workspace(conv, n, log2r) bytes."""
        self._fm_rx_c16("cordic_plan_fm_rx_decim_c16",
                        self.fm_rx_decim_c16_workspace, (log2r,), conv, fcw, iq,
                        mag, freq, work, pm, n, phase0, acc, dphase0, last,
                        stream)

    @property
    def queue_info(self):
        """tile-queue ring of the handle (include/cordic_amd.h)"""
        return _queue_info("cordic_plan_queue_info", self._h)

    def prepare(self, x0, y0, stream=None):
        """build the seed image of the constant vector (x0, y0) now"""
        _check(lib().cordic_plan_prepare(self._h, x0, y0, _stream(stream)),
               "cordic_plan_prepare")

    @property
    def image_info(self):
        """seed images the plan holds; launches served from one / not"""
        a, b, c = C.c_int32(), C.c_uint64(), C.c_uint64()
        _check(lib().cordic_plan_image_info(self._h, C.byref(a), C.byref(b),
                                            C.byref(c)),
               "cordic_plan_image_info")
        return dict(held=a.value, hits=b.value, misses=c.value)

    def p2r_const_batch(self, jobs, x0, y0, stream=None):
        """one-shot batch of phase-array jobs (cordic_plan_p2r_const_batch)"""
        _check(lib().cordic_plan_p2r_const_batch(
            self._h, len(jobs), _job_array(jobs), x0, y0, _stream(stream)),
            "cordic_plan_p2r_const_batch")

    def nco_batch(self, jobs, x0, y0, stream=None):
        _check(lib().cordic_plan_nco_batch(
            self._h, len(jobs), _job_array(jobs), x0, y0, _stream(stream)),
            "cordic_plan_nco_batch")

    def xy_batch(self, kind, jobs, stream=None):
        """one-shot batch of data-fed jobs (cordic_plan_r2p_batch / _p2r_batch
        / _mix_batch by kind)"""
        name = {JOBS_R2P: "cordic_plan_r2p_batch",
                JOBS_P2R_XY: "cordic_plan_p2r_batch",
                JOBS_MIX: "cordic_plan_mix_batch"}[kind]
        _check(getattr(lib(), name)(self._h, len(jobs), _job_array(jobs),
                                    _stream(stream)), name)

    def set_min_samples(self, n):
        """batch size from which the table-driven kernels serve (< 0: default)"""
        _check(lib().cordic_plan_set_min_samples(self._h, n),
               "cordic_plan_set_min_samples")

    @property
    def tail_groups(self):
        """stages per looked-up group behind the seeds ([] = no direction tails)"""
        n = C.c_int32()
        st = (C.c_int32 * 4)()
        _check(lib().cordic_plan_tail_info(self._h, C.byref(n), st),
               "cordic_plan_tail_info")
        return [int(st[g]) for g in range(n.value)]

    def p2r_const(self, x0, y0, phase, ox, oy, n=None, stream=None):
        n = phase.numel() if n is None else n
        if _is16(ox):
            _same16("cordic_plan_p2r16_const", phase, ox, oy)
            _check(lib().cordic_plan_p2r16_const(
                self._h, n, x0, y0, _ptr(phase), _ptr(ox), _ptr(oy),
                _stream(stream)), "cordic_plan_p2r16_const")
            return
        _check(lib().cordic_plan_p2r_const(self._h, n, x0, y0, _ptr(phase),
                                           _ptr(ox), _ptr(oy),
                                           _stream(stream)),
               "cordic_plan_p2r_const")

    def nco(self, n, phase0, fcw, index0, x0, y0, ox, oy, stream=None):
        if _is16(ox):
            _same16("cordic_plan_nco16", ox, oy)
            _check(lib().cordic_plan_nco16(
                self._h, n, phase0 & 0xffffffff, fcw & 0xffffffff, index0,
                x0, y0, _ptr(ox), _ptr(oy), _stream(stream)),
                "cordic_plan_nco16")
            return
        _check(lib().cordic_plan_nco(self._h, n, phase0 & 0xffffffff,
                                     fcw & 0xffffffff, index0, x0, y0,
                                     _ptr(ox), _ptr(oy), _stream(stream)),
               "cordic_plan_nco")


class _CJob(C.Structure):
    _fields_ = [("d_phase", C.c_void_p), ("phase0", C.c_uint32),
                ("fcw", C.c_uint32), ("index0", C.c_uint64),
                ("d_oxval", C.c_void_p), ("d_oyval", C.c_void_p),
                ("n", C.c_uint64),
                ("d_xval", C.c_void_p), ("d_yval", C.c_void_p)]


class _CJob16(_CJob):
    """cordic_job16: cordic_job whose sample pointers are int16_t / uint16_t
    ones -- the same fields at the same offsets"""


JOBS_PHASE_ARRAYS, JOBS_NCO, JOBS_R2P, JOBS_P2R_XY, JOBS_MIX = 0, 1, 2, 3, 4
# enum cordic_jobs_path: how the latest run of a set went
JOBS_PATH_NONE, JOBS_PATH_FUSED, JOBS_PATH_ONE_BY_ONE = 0, 1, 2


def _jobs_are16(jobs):
    """True: every sample tensor of the jobs is 16-bit (cordic_job16), False:
    none is; a mixture is refused"""
    sizes = {t.element_size() for jb in jobs
             for t in (jb.get(k) for k in ("phase", "x", "y", "ox", "oy"))
             if hasattr(t, "element_size")}
    if 2 in sizes and len(sizes) > 1:
        raise TypeError("job set: 16-bit and wider sample arrays in one set")
    return sizes == {2}


def _job_array(jobs, ctype=_CJob):
    """jobs: dicts with phase (tensor or None), ox, oy, n; for NCO / MIX jobs
    phase0, fcw, index0; for the data-fed kinds x, y (R2P: ox = o_mag, oy =
    o_phase) -> a C array of cordic_job (ctype=_CJob16: of cordic_job16)"""
    arr = (ctype * max(1, len(jobs)))()
    for k, jb in enumerate(jobs):
        ph = jb.get("phase")
        arr[k].d_phase = _ptr(ph) if ph is not None else None
        arr[k].phase0 = jb.get("phase0", 0) & 0xffffffff
        arr[k].fcw = jb.get("fcw", 0) & 0xffffffff
        arr[k].index0 = jb.get("index0", 0)
        arr[k].d_oxval = _ptr(jb["ox"])
        arr[k].d_oyval = _ptr(jb["oy"])
        arr[k].n = jb["n"]
        for key, field in (("x", "d_xval"), ("y", "d_yval")):
            v = jb.get(key)
            setattr(arr[k], field, _ptr(v) if v is not None else None)
    return arr


class Jobset:
    """cordic_jobset: many small jobs cut into tiles once, run in one launch."""

    def __init__(self, plan, kind, jobs):
        self.plan = plan
        self._keep = jobs          # the tensors behind the addresses
        h = C.c_void_p()
        self.io16 = _jobs_are16(jobs)
        if self.io16:      # int16 / uint16 tensors: cordic_job16
            _check(lib().cordic_jobset_create16(
                plan._h, kind, len(jobs), _job_array(jobs, _CJob16),
                C.byref(h)), "cordic_jobset_create16")
        else:
            _check(lib().cordic_jobset_create(
                plan._h, kind, len(jobs), _job_array(jobs), C.byref(h)),
                "cordic_jobset_create")
        self._h = h

    @property
    def info(self):
        a, b, c = C.c_uint64(), C.c_uint32(), C.c_uint32()
        _check(lib().cordic_jobset_info(self._h, C.byref(a), C.byref(b),
                                        C.byref(c)), "cordic_jobset_info")
        return dict(samples=a.value, tiles=b.value, tail_samples=c.value)

    @property
    def path(self):
        """JOBS_PATH_NONE before the first run, else JOBS_PATH_FUSED or
        JOBS_PATH_ONE_BY_ONE: the way the latest run went"""
        p = C.c_int32()
        _check(lib().cordic_jobset_path(self._h, C.byref(p)),
               "cordic_jobset_path")
        return p.value

    def run(self, x0=0, y0=0, stream=None, plan=None):
        _check(lib().cordic_plan_run_jobs((plan or self.plan)._h, self._h, x0,
                                          y0, _stream(stream)),
               "cordic_plan_run_jobs")

    def close(self):
        if getattr(self, "_h", None):
            lib().cordic_jobset_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def jobset_reap():
    lib().cordic_jobset_reap()


class Group:
    """cordic_group: the local shards of a multi-GPU job (include/
    cordic_amd.h, "multi-GPU jobs").  devices=None: ordinals 0..nlocal-1."""

    IN0, IN1, OUT0, OUT1 = 0, 1, 2, 3

    def __init__(self, cfg, nlocal=1, devices=None, first_shard=0,
                 total_shards=None):
        self.cfg = cfg
        dv = None
        if devices is not None:
            nlocal = len(devices)
            dv = (C.c_int * nlocal)(*devices)
        total = nlocal if total_shards is None else total_shards
        h = C.c_void_p()
        _check(lib().cordic_group_create(cfg.ref, nlocal, dv, first_shard,
                                         total, C.byref(h)),
               "cordic_group_create")
        self._h = h
        self.nlocal, self.first, self.total = nlocal, first_shard, total

    def close(self):
        if getattr(self, "_h", None):
            lib().cordic_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def range(self, n_total, shard):
        a, c = C.c_uint64(), C.c_uint64()
        _check(lib().cordic_group_range(self._h, n_total, shard, C.byref(a),
                                        C.byref(c)), "cordic_group_range")
        return a.value, c.value

    def reserve(self, n_total, inputs):
        _check(lib().cordic_group_reserve(self._h, n_total, inputs),
               "cordic_group_reserve")

    def fill_phase_ramp(self, n_total, shift):
        _check(lib().cordic_group_fill_phase_ramp(self._h, n_total, shift),
               "cordic_group_fill_phase_ramp")

    def fill_iq_ramp(self, n_total, mulx, muly, bits):
        _check(lib().cordic_group_fill_iq_ramp(self._h, n_total, mulx, muly,
                                               bits),
               "cordic_group_fill_iq_ramp")

    def p2r_const(self, n_total, x0, y0):
        _check(lib().cordic_group_p2r_const(self._h, n_total, x0, y0),
               "cordic_group_p2r_const")

    def nco(self, n_total, phase0, fcw, x0, y0):
        _check(lib().cordic_group_nco(self._h, n_total, phase0 & 0xffffffff,
                                      fcw & 0xffffffff, x0, y0),
               "cordic_group_nco")

    def r2p(self, n_total):
        _check(lib().cordic_group_r2p(self._h, n_total), "cordic_group_r2p")

    def sync(self):
        _check(lib().cordic_group_sync(self._h), "cordic_group_sync")

    def digest(self, n_total):
        d = C.c_uint64()
        _check(lib().cordic_group_digest(self._h, n_total, C.byref(d)),
               "cordic_group_digest")
        return d.value

    def set_gather(self, root_device, out0=None, out1=None, chunks=8):
        """out0 / out1: device tensors or raw device addresses."""
        def addr(t):
            return t if isinstance(t, int) or t is None else _ptr(t)
        _check(lib().cordic_group_set_gather(self._h, root_device, addr(out0),
                                             addr(out1), chunks),
               "cordic_group_set_gather")

    def set_placement(self, enable):
        """False / 0: off (the default); True / 1: two spare arrays; N >= 2:
        up to N spares while no written pair is fast (include/cordic_amd.h)"""
        _check(lib().cordic_group_set_placement(self._h, int(enable)),
               "cordic_group_set_placement")

    def placement(self, local_shard=0):
        """What the last allocation of the shard's arrays saw."""
        c, p = C.c_int(), C.c_int()
        wb, ww, b, w = (C.c_float() for _ in range(4))
        _check(lib().cordic_group_placement(self._h, local_shard, C.byref(c),
                                            C.byref(p), C.byref(wb),
                                            C.byref(ww), C.byref(b),
                                            C.byref(w)),
               "cordic_group_placement")
        return {"candidates": c.value, "probes": p.value,
                "written_pair_best_ms": wb.value,
                "written_pair_worst_ms": ww.value,
                "best_ms": b.value, "worst_ms": w.value}

    def rccl_init(self, unique_id):
        """Join the job's RCCL communicator (collective over all shards);
        unique_id: the 128 bytes of rccl_unique_id() from one process."""
        if len(unique_id) != RCCL_ID_BYTES:
            raise ValueError("an RCCL unique id is %d bytes" % RCCL_ID_BYTES)
        buf = C.create_string_buffer(bytes(unique_id), RCCL_ID_BYTES)
        _check(lib().cordic_group_rccl_init(self._h, buf),
               "cordic_group_rccl_init")

    def set_gather_rccl(self, root_shard, out0=None, out1=None, chunks=8):
        """out0 / out1 (root's process only): device tensors or addresses."""
        def addr(t):
            return t if isinstance(t, int) or t is None else _ptr(t)
        _check(lib().cordic_group_set_gather_rccl(self._h, root_shard,
                                                  addr(out0), addr(out1),
                                                  chunks),
               "cordic_group_set_gather_rccl")

    def mark(self, slot):
        _check(lib().cordic_group_mark(self._h, slot), "cordic_group_mark")

    def elapsed(self, a, b):
        """(max over the local shards, [per shard]) in ms."""
        mx = C.c_float()
        per = (C.c_float * self.nlocal)()
        _check(lib().cordic_group_elapsed(self._h, a, b, C.byref(mx), per),
               "cordic_group_elapsed")
        return mx.value, list(per)

    def buffers(self, local_shard):
        dev = C.c_int()
        p = [C.c_void_p() for _ in range(4)]
        cap = C.c_uint64()
        _check(lib().cordic_group_buffers(self._h, local_shard, C.byref(dev),
                                          *[C.byref(q) for q in p],
                                          C.byref(cap)),
               "cordic_group_buffers")
        return dev.value, [q.value for q in p], cap.value

    def read(self, local_shard, array, offset, count, dtype=None):
        import numpy as np
        out = np.empty(count, dtype=np.int32 if dtype is None else dtype)
        _check(lib().cordic_group_read(self._h, local_shard, array, offset,
                                       count, out.ctypes.data), "cordic_group_read")
        return out

    def read_into(self, local_shard, array, offset, dst):
        """dst: device tensor (or numpy array) of 32-bit words to fill."""
        if hasattr(dst, "ctypes"):
            addr, count = dst.ctypes.data, dst.size
        else:
            addr, count = _ptr(dst), dst.numel()
        _check(lib().cordic_group_read(self._h, local_shard, array, offset,
                                       count, addr), "cordic_group_read")

    def write(self, local_shard, array, offset, src):
        """src: numpy array (host) or device tensor of 32-bit words."""
        if hasattr(src, "ctypes"):
            addr, count = src.ctypes.data, src.size
        else:
            addr, count = _ptr(src), src.numel()
        _check(lib().cordic_group_write(self._h, local_shard, array, offset,
                                        count, addr), "cordic_group_write")


class Arrays:
    """cordic_arrays_alloc: n_read + n_write device arrays of `nbytes` bytes
    (plain hipMalloc; placed by measurement with CORDIC_GROUP_PLACEMENT=1 in
    the environment: include/cordic_amd.h, "Placement"), as torch tensor views;
    read arrays first."""

    class _View:
        def __init__(self, ptr, count, typestr):
            self.__cuda_array_interface__ = {
                "shape": (count,), "typestr": typestr, "data": (ptr, False),
                "version": 2}

    def __init__(self, nbytes, n_read, n_write, stream=None):
        self.nbytes, self.count = int(nbytes), n_read + n_write
        self._p = (C.c_void_p * self.count)()
        _check(lib().cordic_arrays_alloc(self.nbytes, n_read, n_write, self._p,
                                         stream), "cordic_arrays_alloc")
        self.ptrs = [int(self._p[i]) for i in range(self.count)]

    def tensor(self, k, dtype):
        import torch
        code = {torch.int32: "<i4", torch.int16: "<i2"}[dtype]
        per = 4 if dtype == torch.int32 else 2
        return torch.as_tensor(Arrays._View(self.ptrs[k], self.nbytes // per, code),
                               device="cuda")

    def close(self):
        if getattr(self, "_p", None) is not None:
            lib().cordic_arrays_free(self._p, self.count)
            self._p = None

    def __del__(self):
        self.close()


RCCL_ID_BYTES = 128


def rccl_unique_id():
    """128 bytes for Group.rccl_init, from ONE process of the job."""
    buf = C.create_string_buffer(RCCL_ID_BYTES)
    _check(lib().cordic_rccl_unique_id(buf), "cordic_rccl_unique_id")
    return buf.raw


def device_count():
    return lib().cordic_device_count()


def shard_range(n_total, shard, total_shards):
    a, c = C.c_uint64(), C.c_uint64()
    _check(lib().cordic_shard_range(n_total, shard, total_shards, C.byref(a),
                                    C.byref(c)), "cordic_shard_range")
    return a.value, c.value


TBL, QTR = 4, 5


class _CTableConfig(C.Structure):
    _fields_ = [("kind", C.c_int32), ("pw", C.c_int32), ("ow", C.c_int32),
                ("entries", C.c_int32)]


class _CQueueInfo(C.Structure):
    _fields_ = [("eager_slots", C.c_int32), ("captured_capacity", C.c_int32),
                ("captured_used", C.c_int32), ("fallback_launches", C.c_uint64)]


def _queue_info(fn, handle):
    q = _CQueueInfo()
    _check(getattr(lib(), fn)(handle, C.byref(q)), fn)
    return {k: int(getattr(q, k)) for k, _ in _CQueueInfo._fields_}


def _osc_nco(fn, handle, sin, cos, n, phase0, fcw, index0, stream):
    n = sin.numel() if n is None else n
    if _is16(sin) or _is16(cos):
        fn += "16"
        _same16(fn, sin, cos)
    _check(getattr(lib(), fn)(handle, n, phase0 & 0xffffffff, fcw & 0xffffffff,
                              index0 & 0xffffffffffffffff, _ptr(sin), _ptr(cos),
                              _stream(stream)), fn)


def fm_workspace(n):
    """cordic_fm_workspace: bytes of device scratch a modulated oscillator
    call of n samples needs (16-byte aligned)"""
    return int(lib().cordic_fm_workspace(n))


def _fm_work(work, n):
    """The caller owns the scratch, as in the C ABI: it has to outlive the
    call on the stream, which only the caller can see to."""
    if work is None and n:
        raise TypeError("work: a device buffer of fm_workspace(n) bytes")
    return work


def phase_accumulate(fcw, phase, pm=None, n=None, phase0=0, acc=None,
                     work=None, stream=None):
    """cordic_phase_accumulate: phase[i] = phase0 + acc[0] + fcw[0] + .. +
    fcw[i-1] + pm[i] (mod 2^32); acc (a one-word device tensor, optional)
    carries the sum from call to call; phase may be fcw itself.  work: device
    scratch of fm_workspace(n) bytes (16-byte aligned), the caller's."""
    n = fcw.numel() if n is None else n
    work = _fm_work(work, n)
    st = _stream(stream)
    _check(lib().cordic_phase_accumulate(n, _ptr(fcw), _ptr(pm),
                                         phase0 & 0xffffffff, _ptr(acc),
                                         _ptr(phase), _ptr(work), st),
           "cordic_phase_accumulate")


def _osc_fm(fn, handle, fcw, sin, cos, pm, n, phase0, acc, work, stream):
    n = fcw.numel() if n is None else n
    if _is16(sin) or _is16(cos):
        fn += "16"
        _same16(fn, sin, cos)
    work = _fm_work(work, n)
    st = _stream(stream)
    _check(getattr(lib(), fn)(handle, n, _ptr(fcw), _ptr(pm),
                              phase0 & 0xffffffff, _ptr(acc), _ptr(sin),
                              _ptr(cos), _ptr(work), st), fn)


class _COscJob(C.Structure):
    """cordic_osc_job / cordic_osc_job16 (the same layout)"""
    _fields_ = [("phase0", C.c_uint32), ("fcw", C.c_uint32),
                ("index0", C.c_uint64), ("n", C.c_uint64),
                ("d_sin", C.c_void_p), ("d_cos", C.c_void_p)]


class _COscTuning(C.Structure):
    _fields_ = [("phase0", C.c_uint32), ("fcw", C.c_uint32),
                ("index0", C.c_uint64)]


_OSC_KEYS = ("phase0", "fcw", "index0", "n", "sin", "cos")


class OscBank:
    """cordic_oscbank: many oscillator jobs of one Table / Quad core, cut once
    and run as one launch.  jobs: tuples (phase0, fcw, index0, n, sin, cos) or
    dicts with those keys; sin / cos are tensors or device addresses, cos may
    be None (sine only)."""

    def __init__(self, core, fn, jobs, i16=False):
        self.core = core           # the bank must go before its core handle
        jobs = [tuple(jb.get(k) for k in _OSC_KEYS) if isinstance(jb, dict)
                else tuple(jb) for jb in jobs]
        self._keep = jobs          # the tensors behind the addresses
        arr = (_COscJob * max(1, len(jobs)))()
        for k, (phase0, fcw, index0, n, sin, cos) in enumerate(jobs):
            arr[k].phase0 = (phase0 or 0) & 0xffffffff
            arr[k].fcw = (fcw or 0) & 0xffffffff
            arr[k].index0 = (index0 or 0) & 0xffffffffffffffff
            arr[k].n = n
            arr[k].d_sin = _ptr(sin)
            arr[k].d_cos = _ptr(cos)
        fn += "16" if i16 else ""
        h = C.c_void_p()
        _check(getattr(lib(), fn)(core._h, len(jobs), arr, C.byref(h)), fn)
        self._h = h

    def info(self):
        a, b, c = C.c_uint64(), C.c_uint32(), C.c_uint32()
        _check(lib().cordic_oscbank_info(self._h, C.byref(a), C.byref(b),
                                         C.byref(c)), "cordic_oscbank_info")
        return dict(samples=a.value, tiles=b.value, edge_samples=c.value)

    def run(self, index_offset=0, stream=None):
        _check(lib().cordic_oscbank_run(
            self._h, index_offset & 0xffffffffffffffff, _stream(stream)),
            "cordic_oscbank_run")

    def retune(self, first, tunings, stream=None):
        """tunings: (phase0, fcw, index0) of jobs first, first + 1, ..."""
        arr = (_COscTuning * max(1, len(tunings)))()
        for k, (phase0, fcw, index0) in enumerate(tunings):
            arr[k].phase0 = phase0 & 0xffffffff
            arr[k].fcw = fcw & 0xffffffff
            arr[k].index0 = index0 & 0xffffffffffffffff
        _check(lib().cordic_oscbank_retune(self._h, first, len(tunings), arr,
                                           _stream(stream)),
               "cordic_oscbank_retune")

    def close(self):
        if getattr(self, "_h", None):
            lib().cordic_oscbank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CFmOscJob(C.Structure):
    """cordic_fmosc_job / cordic_fmosc_job16 (the same layout)"""
    _fields_ = [("d_fcw", C.c_void_p), ("d_pm", C.c_void_p),
                ("d_sin", C.c_void_p), ("d_cos", C.c_void_p),
                ("d_acc", C.c_void_p), ("n", C.c_uint64),
                ("phase0", C.c_uint32), ("reserved", C.c_uint32)]


_FMOSC_KEYS = ("fcw", "pm", "sin", "cos", "n", "phase0", "acc")


class FmBank:
    """cordic_fmbank: many fm jobs of one Table / Quad core, cut once and run
    in two launches.  jobs: tuples (fcw, pm, sin, cos, n, phase0, acc) or dicts
    with those keys; fcw is an int32 tensor or a device address, pm one more or
    None, sin / cos int32 tensors (int16 with i16) or device addresses, cos
    None: sine only, acc a one-word device tensor or None; n None:
    fcw.numel().  The core must stay open as long as the bank."""

    def __init__(self, core, fn, jobs, i16=False):
        jobs = [tuple(jb.get(k) for k in _FMOSC_KEYS) if isinstance(jb, dict)
                else tuple(jb) for jb in jobs]
        self._keep = (core, jobs)   # the core and the tensors behind the addresses
        arr = (_CFmOscJob * max(1, len(jobs)))()
        for k, (fcw, pm, sin, cos, n, phase0, acc) in enumerate(jobs):
            if i16:
                _same16(fn + "16", sin, cos)
            arr[k].d_fcw = _ptr(fcw)
            arr[k].d_pm = _ptr(pm)
            arr[k].d_sin = _ptr(sin)
            arr[k].d_cos = _ptr(cos)
            arr[k].d_acc = _ptr(acc)
            arr[k].n = fcw.numel() if n is None else n
            arr[k].phase0 = (phase0 or 0) & 0xffffffff
        fn += "16" if i16 else ""
        h = C.c_void_p()
        _check(getattr(lib(), fn)(core._h, len(jobs), arr, C.byref(h)), fn)
        self._h = h

    def info(self):
        a, b, c = C.c_uint64(), C.c_uint32(), C.c_int32()
        _check(lib().cordic_fmbank_info(self._h, C.byref(a), C.byref(b),
                                        C.byref(c)), "cordic_fmbank_info")
        return dict(samples=a.value, spans=b.value, tile=c.value)

    def run(self, stream=None):
        _check(lib().cordic_fmbank_run(self._h, _stream(stream)),
               "cordic_fmbank_run")

    def close(self):
        if getattr(self, "_h", None):
            lib().cordic_fmbank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Table:
    """A -t tbl / -t qtr core: cordic_table_config + its device table."""

    def __init__(self, kind, iw=-1, ow=-1, pw=-1, device=True):
        self.c = _CTableConfig()
        _check(lib().cordic_table_config_init(C.byref(self.c), kind, iw, ow,
                                              pw), "cordic_table_config_init")
        self._h = None
        if device:
            h = C.c_void_p()
            _check(lib().cordic_table_create(C.byref(self.c), C.byref(h)),
                   "cordic_table_create")
            self._h = h

    pw = property(lambda self: self.c.pw)
    ow = property(lambda self: self.c.ow)
    entries = property(lambda self: self.c.entries)

    def values(self):
        import numpy as np
        out = np.empty(self.c.entries, dtype=np.int32)
        _check(lib().cordic_table_values(C.byref(self.c),
                                         out.ctypes.data_as(_i32p), out.size),
               "cordic_table_values")
        return out

    @property
    def lds_mode(self):
        return lib().cordic_table_lds_mode(self._h)

    @property
    def queue_info(self):
        return _queue_info("cordic_table_queue_info", self._h)

    def lookup(self, phase, val, n=None, stream=None):
        n = phase.numel() if n is None else n
        _check(lib().cordic_table_lookup(self._h, n, _ptr(phase), _ptr(val),
                                         _stream(stream)),
               "cordic_table_lookup")

    def nco(self, sin, cos=None, n=None, phase0=0, fcw=1, index0=0,
            stream=None):
        """cordic_table_nco: sin[i] = the core at phase0 + (index0 + i) * fcw,
        cos[i] = the core a quarter turn ahead (None: sine only); int16
        tensors take the 16-bit entry point."""
        _osc_nco("cordic_table_nco", self._h, sin, cos, n, phase0, fcw, index0,
                 stream)

    def fm(self, fcw, sin, cos=None, pm=None, n=None, phase0=0, acc=None,
           work=None, stream=None):
        """cordic_table_fm: the oscillator with one tuning word per sample,
        sin[i] = the core at phase0 + acc[0] + fcw[0] + .. + fcw[i-1] + pm[i],
        cos[i] a quarter turn ahead (None: sine only); acc: optional one-word
        device tensor that carries the accumulator from call to call; int16
        tensors take the 16-bit entry point.  work: device scratch of
        fm_workspace(n) bytes (16-byte aligned), the caller's."""
        _osc_fm("cordic_table_fm", self._h, fcw, sin, cos, pm, n, phase0, acc,
                work, stream)

    def bank(self, jobs, i16=False):
        """cordic_table_bank_create(16): the jobs as one OscBank"""
        return OscBank(self, "cordic_table_bank_create", jobs, i16)

    def fm_bank(self, jobs, i16=False):
        """cordic_table_fmbank_create(16): the fm jobs as one FmBank"""
        return FmBank(self, "cordic_table_fmbank_create", jobs, i16)

    def close(self):
        if self._h:
            lib().cordic_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CQuadConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "pw", "ow", "xtra", "tbl_width", "ww", "lgtbl", "entries", "dxbits",
        "cbits", "lbits", "qbits", "has_reset", "has_aux")] + [
        ("scale", C.c_int64), ("itbl_err", C.c_double),
        ("tbl_err", C.c_double), ("spur_db", C.c_double)]


class Quad:
    """A -t qtbl core (quadratically interpolated sine): cordic_quad_config +
    its device tables.  from_cli mirrors gencordic's flags; from_core the
    emitter's (phase_bits, ow, nxtra) tuple."""

    def __init__(self, iw=-1, ow=-1, xtra=2, pw=-1, device=True, core=None):
        self.c = _CQuadConfig()
        if core is not None:
            _check(lib().cordic_quad_config_init_core(C.byref(self.c), *core),
                   "cordic_quad_config_init_core")
        else:
            _check(lib().cordic_quad_config_init(C.byref(self.c), iw, ow, xtra,
                                                 pw), "cordic_quad_config_init")
        self._h = None
        if device:
            h = C.c_void_p()
            _check(lib().cordic_quad_create(C.byref(self.c), C.byref(h)),
                   "cordic_quad_create")
            self._h = h

    def __getattr__(self, name):
        if name in ("c", "_h"):
            raise AttributeError(name)
        return getattr(self.c, name)

    def tables(self):
        import numpy as np
        out = [np.empty(self.c.entries, dtype=np.int32) for _ in range(3)]
        _check(lib().cordic_quad_tables(
            C.byref(self.c), *[o.ctypes.data_as(_i32p) for o in out],
            self.c.entries), "cordic_quad_tables")
        return out

    def header(self, name="quadtbl"):
        buf = C.create_string_buffer(4096)
        n = lib().cordic_quad_write_header(C.byref(self.c), name.encode(), buf,
                                           4096)
        if n < 0:
            raise CordicError(n, "cordic_quad_write_header")
        return buf.value.decode()

    @property
    def queue_info(self):
        return _queue_info("cordic_quad_queue_info", self._h)

    def lookup(self, phase, val, n=None, stream=None):
        n = phase.numel() if n is None else n
        _check(lib().cordic_quad_lookup(self._h, n, _ptr(phase), _ptr(val),
                                        _stream(stream)), "cordic_quad_lookup")

    def nco(self, sin, cos=None, n=None, phase0=0, fcw=1, index0=0,
            stream=None):
        """cordic_quad_nco: as Table.nco with o_sin of this core"""
        _osc_nco("cordic_quad_nco", self._h, sin, cos, n, phase0, fcw, index0,
                 stream)

    def fm(self, fcw, sin, cos=None, pm=None, n=None, phase0=0, acc=None,
           work=None, stream=None):
        """cordic_quad_fm: as Table.fm with o_sin of this core"""
        _osc_fm("cordic_quad_fm", self._h, fcw, sin, cos, pm, n, phase0, acc,
                work, stream)

    def bank(self, jobs, i16=False):
        """cordic_quad_bank_create(16): the jobs as one OscBank"""
        return OscBank(self, "cordic_quad_bank_create", jobs, i16)

    def fm_bank(self, jobs, i16=False):
        """cordic_quad_fmbank_create(16): the fm jobs as one FmBank"""
        return FmBank(self, "cordic_quad_fmbank_create", jobs, i16)

    def close(self):
        if self._h:
            lib().cordic_quad_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Stream:
    """cordic_stream: a pipelined core (p2r / r2p) stepped in blocks of clocks
    with per-clock i_ce / i_reset / i_aux, pipeline state carried between
    calls (include/cordic_amd.h, "clocked view")."""

    def __init__(self, cfg):
        self.cfg = cfg
        h = C.c_void_p()
        _check(lib().cordic_stream_create(cfg.ref, C.byref(h)),
               "cordic_stream_create")
        self._h = h

    @property
    def latency(self):
        return lib().cordic_stream_latency(self._h)

    def reserve(self, ticks):
        _check(lib().cordic_stream_reserve(self._h, ticks),
               "cordic_stream_reserve")

    def reset(self, stream=None):
        _check(lib().cordic_stream_reset(self._h, _stream(stream)),
               "cordic_stream_reset")

    def ticks(self, x, y, phase, out0, out1, oaux=None, ce=None, reset=None,
              aux=None, n=None, stream=None):
        n = x.numel() if n is None else n
        _check(lib().cordic_stream_ticks(
            self._h, n, _ptr(ce), _ptr(reset), _ptr(aux), _ptr(x), _ptr(y),
            _ptr(phase), _ptr(out0), _ptr(out1), _ptr(oaux), _stream(stream)),
            "cordic_stream_ticks")

    def close(self):
        if self._h:
            lib().cordic_stream_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Seq:
    """cordic_seq: a sequential core (sp2r / sr2p) behind its i_stb / o_busy /
    o_done handshake, stepped in blocks of clocks."""

    def __init__(self, cfg):
        self.cfg = cfg
        h = C.c_void_p()
        _check(lib().cordic_seq_create(cfg.ref, C.byref(h)), "cordic_seq_create")
        self._h = h

    def ticks(self, stb, x, y, phase, out0, out1, busy=None, done=None,
              oaux=None, reset=None, aux=None, n=None, stream=None):
        n = stb.numel() if n is None else n
        _check(lib().cordic_seq_ticks(
            self._h, n, _ptr(stb), _ptr(reset), _ptr(aux), _ptr(x), _ptr(y),
            _ptr(phase), _ptr(out0), _ptr(out1), _ptr(busy), _ptr(done),
            _ptr(oaux), _stream(stream)), "cordic_seq_ticks")

    @property
    def violations(self):
        v = C.c_uint64()
        _check(lib().cordic_seq_violations(self._h, C.byref(v)),
               "cordic_seq_violations")
        return v.value

    def close(self):
        if self._h:
            lib().cordic_seq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _CP2RQuality(C.Structure):
    _fields_ = ([("n", C.c_uint64)]
                + [(k, C.c_double) for k in (
                    "avg_err", "max_err", "mag", "input_mag", "alpha",
                    "cnr_db", "expected_err", "avg_limit", "max_limit")]
                + [("max_err_index", C.c_uint64)]
                + [(k, C.c_int32) for k in (
                    "pass_avg", "pass_max", "pass_alpha", "pass")]
                + [(k, C.c_double) for k in (
                    "sum_err2", "sum_xy", "sum_sq", "sum_d", "sum_in2")])


class _CR2PQuality(C.Structure):
    _fields_ = ([("n", C.c_uint64)]
                + [(k, C.c_double) for k in (
                    "max_phase_err", "max_mag_err", "avg_phase_err",
                    "avg_mag_err", "mean_phase_err",
                    "expected_avg_phase_err", "phase_limit", "mag_limit")]
                + [("max_phase_err_index", C.c_uint64),
                   ("max_mag_err_index", C.c_uint64)]
                + [(k, C.c_int32) for k in (
                    "pass_phase", "pass_mag", "pass")])


class _CSineQuality(C.Structure):
    _fields_ = [("n", C.c_uint64), ("max_err", C.c_double),
                ("max_err_index", C.c_uint64), ("max_err_phase", C.c_uint32),
                ("max_val", C.c_int32), ("min_val", C.c_int32),
                ("scale", C.c_double), ("tbl_err", C.c_double),
                ("limit", C.c_double), ("judged", C.c_int32),
                ("pass", C.c_int32)]


class _CSfdrResult(C.Structure):
    _fields_ = [("n", C.c_uint64), ("master", C.c_double),
                ("spur", C.c_double), ("spur_bin", C.c_uint64),
                ("sfdr_dbc", C.c_double)]


def _as_dict(st):
    return {k: getattr(st, k) for k, _ in st._fields_}


class Quality:
    """cordic_quality: the reference benches' statistics and thresholds
    (bench/cpp/cordic_tb.cpp:223-337, topolar_tb.cpp:222-315), reduced on the
    device; calls accumulate until reset()."""

    def __init__(self, cfg, _create="cordic_quality_create"):
        self.cfg = cfg
        self._h = C.c_void_p()
        # (Quad / Table objects carry their config struct as .c)
        ref = cfg.ref if hasattr(cfg, "ref") else C.byref(getattr(cfg, "c", cfg))
        _check(getattr(lib(), _create)(ref, C.byref(self._h)), _create)

    @classmethod
    def for_quad(cls, quadcfg):
        """statistics of a -t qtbl core (a Quad or its cordic_quad_config):
        sine(), sine_nco(), sine_result()"""
        return cls(quadcfg, "cordic_quality_create_quad")

    @classmethod
    def for_table(cls, tablecfg):
        """the same for a -t tbl / -t qtr core (a Table or its config); the
        reference has no threshold for these: judged = 0"""
        return cls(tablecfg, "cordic_quality_create_table")

    def reset(self, stream=None):
        _check(lib().cordic_quality_reset(self._h, _stream(stream)),
               "cordic_quality_reset")

    def p2r(self, x, y, phase, ox, oy, n=None, stream=None):
        """x, y: ints (the constant vector) or int32 tensors"""
        n = phase.numel() if n is None else n
        if isinstance(x, int):
            a = (None, None, x, y)
        else:
            a = (_ptr(x), _ptr(y), 0, 0)
        _check(lib().cordic_quality_p2r(self._h, n, a[0], a[1], a[2], a[3],
                                        _ptr(phase), _ptr(ox), _ptr(oy),
                                        _stream(stream)),
               "cordic_quality_p2r")

    def nco(self, n, phase0, fcw, index0, x0, y0, ox, oy, stream=None):
        _check(lib().cordic_quality_nco(self._h, n, phase0 & 0xffffffff,
                                        fcw & 0xffffffff, index0, x0, y0,
                                        _ptr(ox), _ptr(oy), _stream(stream)),
               "cordic_quality_nco")

    def r2p(self, x, y, imag, omag, ophase, n=None, stream=None):
        n = x.numel() if n is None else n
        _check(lib().cordic_quality_r2p(self._h, n, _ptr(x), _ptr(y), imag,
                                        _ptr(omag), _ptr(ophase),
                                        _stream(stream)),
               "cordic_quality_r2p")

    def sine(self, phase, val, n=None, stream=None):
        """outputs of *_lookup on a phase array; int16 values take the 16-bit
        entry point"""
        n = phase.numel() if n is None else n
        fn = "cordic_quality_sine16" if _is16(val) else "cordic_quality_sine"
        _check(getattr(lib(), fn)(self._h, n, _ptr(phase), _ptr(val),
                                  _stream(stream)), fn)

    def sine_nco(self, val, n=None, phase0=0, fcw=1, index0=0, stream=None):
        """outputs of *_nco / *_nco16 / a bank's job (a cos array: phase0 +
        2^(PW-2)); int16 values take the 16-bit entry point"""
        n = val.numel() if n is None else n
        fn = ("cordic_quality_sine_nco16" if _is16(val)
              else "cordic_quality_sine_nco")
        _check(getattr(lib(), fn)(self._h, n, phase0 & 0xffffffff,
                                  fcw & 0xffffffff,
                                  index0 & 0xffffffffffffffff, _ptr(val),
                                  _stream(stream)), fn)

    def sine_result(self, raw=False):
        """dict of cordic_sine_quality (raw: the struct's bytes)"""
        r = _CSineQuality()
        _check(lib().cordic_quality_sine_result(self._h, C.byref(r)),
               "cordic_quality_sine_result")
        return bytes(r) if raw else _as_dict(r)

    def p2r_result(self):
        r = _CP2RQuality()
        _check(lib().cordic_quality_p2r_result(self._h, C.byref(r)),
               "cordic_quality_p2r_result")
        return _as_dict(r)

    def r2p_result(self):
        r = _CR2PQuality()
        _check(lib().cordic_quality_r2p_result(self._h, C.byref(r)),
               "cordic_quality_r2p_result")
        return _as_dict(r)

    def close(self):
        if self._h:
            lib().cordic_quality_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Sfdr:
    """cordic_sfdr: 2^lgn complex doubles on the device, a forward fp64 FFT
    and the reference benches' spur search (cordic_tb.cpp:340-371,
    quadtbl_tb.cpp:185-219)."""

    def __init__(self, lgn):
        self.lgn = lgn
        self._h = C.c_void_p()
        _check(lib().cordic_sfdr_create(lgn, C.byref(self._h)),
               "cordic_sfdr_create")

    def load_iq(self, re, im, index0=0, n=None, stream=None):
        n = re.numel() if n is None else n
        _check(lib().cordic_sfdr_load_iq(self._h, n, index0, _ptr(re),
                                         _ptr(im), _stream(stream)),
               "cordic_sfdr_load_iq")

    def load_sine(self, sin, index0=0, n=None, stream=None):
        n = sin.numel() if n is None else n
        _check(lib().cordic_sfdr_load_sine(self._h, n, index0, _ptr(sin),
                                           _stream(stream)),
               "cordic_sfdr_load_sine")

    def run(self, stream=None):
        r = _CSfdrResult()
        _check(lib().cordic_sfdr_run(self._h, C.byref(r), _stream(stream)),
               "cordic_sfdr_run")
        return _as_dict(r)

    def bins(self, first=0, count=None):
        """bins of the last transform as a numpy complex128 array"""
        import numpy as np
        count = (1 << self.lgn) - first if count is None else count
        out = np.empty(count, dtype=np.complex128)
        _check(lib().cordic_sfdr_bins(self._h, first, count, out.ctypes.data),
               "cordic_sfdr_bins")
        return out

    def close(self):
        if self._h:
            lib().cordic_sfdr_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fill_circle(x, y, index0, lgnsamples, iw, pw, n=None, stream=None):
    n = x.numel() if n is None else n
    _check(lib().cordic_fill_circle(_ptr(x), _ptr(y), n, index0, lgnsamples,
                                    iw, pw, _stream(stream)),
           "cordic_fill_circle")


KERNEL_GENERIC, KERNEL_UNROLLED, KERNEL_SEEDED, KERNEL_LEFT_JUSTIFIED = 1, 2, 3, 4
KERNEL_DIRECTIONS = 5


def last_kernel():
    """enum cordic_kernel_family of this thread's most recent launch"""
    return lib().cordic_last_kernel()


def seed_table(cfg):
    """Host-side seed table words of a core (numpy uint32) or None."""
    import numpy as np
    cap = 4 + 4096 * 6 + 4 + 4 * (6 + 2 * 4096 + 2 * 256)
    buf = np.zeros(cap, dtype=np.uint32)
    n = lib().cordic_seed_table(cfg.ref, buf.ctypes.data_as(_u32p), cap)
    return buf[:n].copy() if n else None


def dir_table(cfg):
    """Host-side direction tables of the per-sample-vector path (numpy
    uint32 words) or None."""
    import numpy as np
    cap = 4 + 5 * (6 + 2 * 4096 + 2 * 256)
    buf = np.zeros(cap, dtype=np.uint32)
    n = lib().cordic_dir_table(cfg.ref, buf.ctypes.data_as(_u32p), cap)
    return buf[:n].copy() if n else None


def _ptr(t):
    """Device pointer of a torch tensor (or an int / None passed through)."""
    if t is None:
        return None
    if isinstance(t, int):
        return t
    return t.data_ptr()


def _stream(stream):
    if stream is None:
        import torch
        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


def _is16(t):
    """int16 / uint16 sample tensors select the 16-bit-container entry points
    (include/cordic_amd.h: cordic_*16)."""
    return hasattr(t, "element_size") and t.element_size() == 2


def _need_work(work, n, query, *args):
    """The caller's scratch of an FM plan call of n samples: TypeError where
    there is none and n > 0, ValueError where a tensor holds fewer bytes than
    query(*args) answers -- the call's _workspace query, named in both."""
    def asked():
        return "%s(%s)" % (query.__name__, ", ".join(
            str(a) if isinstance(a, int) else "conv" for a in args))
    if work is None and n:
        raise TypeError("work: a device buffer of %s bytes" % asked())
    if hasattr(work, "numel") and hasattr(work, "element_size"):
        have, need = work.numel() * work.element_size(), query(*args)
        if have < need:
            raise ValueError("work: %d bytes, %s = %d" % (have, asked(), need))


def _same16(what, *tensors):
    # (None and raw addresses go through: the library answers for them)
    if any(hasattr(t, "element_size") and t.element_size() != 2 for t in tensors):
        raise TypeError("%s: every sample array must be 16-bit" % what)


def p2r(cfg, x, y, phase, ox, oy, n=None, stream=None):
    n = phase.numel() if n is None else n
    if _is16(ox):
        _same16("cordic_p2r16", x, y, phase, ox, oy)
        _check(lib().cordic_p2r16(cfg.ref, n, _ptr(x), _ptr(y), _ptr(phase),
                                  _ptr(ox), _ptr(oy), _stream(stream)),
               "cordic_p2r16")
        return
    _check(lib().cordic_p2r(cfg.ref, n, _ptr(x), _ptr(y), _ptr(phase),
                            _ptr(ox), _ptr(oy), _stream(stream)), "cordic_p2r")


def p2r_const(cfg, x0, y0, phase, ox, oy, n=None, stream=None):
    n = phase.numel() if n is None else n
    if _is16(ox):
        _same16("cordic_p2r16_const", phase, ox, oy)
        _check(lib().cordic_p2r16_const(cfg.ref, n, x0, y0, _ptr(phase),
                                        _ptr(ox), _ptr(oy), _stream(stream)),
               "cordic_p2r16_const")
        return
    _check(lib().cordic_p2r_const(cfg.ref, n, x0, y0, _ptr(phase), _ptr(ox),
                                  _ptr(oy), _stream(stream)),
           "cordic_p2r_const")


def nco(cfg, n, phase0, fcw, index0, x0, y0, ox, oy, stream=None):
    if _is16(ox):
        _same16("cordic_nco16", ox, oy)
        _check(lib().cordic_nco16(cfg.ref, n, phase0 & 0xffffffff,
                                  fcw & 0xffffffff, index0, x0, y0, _ptr(ox),
                                  _ptr(oy), _stream(stream)), "cordic_nco16")
        return
    _check(lib().cordic_nco(cfg.ref, n, phase0 & 0xffffffff, fcw & 0xffffffff,
                            index0, x0, y0, _ptr(ox), _ptr(oy),
                            _stream(stream)), "cordic_nco")


def mix(cfg, phase0, fcw, index0, x, y, ox, oy, n=None, stream=None):
    """cordic_mix: per-sample x / y rotated by phase0 + (index0 + i) * fcw"""
    n = x.numel() if n is None else n
    if any(_is16(t) for t in (x, y, ox, oy)):
        _same16("cordic_mix16", x, y, ox, oy)
        _check(lib().cordic_mix16(cfg.ref, n, phase0 & 0xffffffff,
                                  fcw & 0xffffffff, index0, _ptr(x), _ptr(y),
                                  _ptr(ox), _ptr(oy), _stream(stream)),
               "cordic_mix16")
        return
    _check(lib().cordic_mix(cfg.ref, n, phase0 & 0xffffffff, fcw & 0xffffffff,
                            index0, _ptr(x), _ptr(y), _ptr(ox), _ptr(oy),
                            _stream(stream)), "cordic_mix")


def r2p(cfg, x, y, mag, ophase, n=None, stream=None):
    n = x.numel() if n is None else n
    if _is16(mag):
        _same16("cordic_r2p16", x, y, mag, ophase)
        _check(lib().cordic_r2p16(cfg.ref, n, _ptr(x), _ptr(y), _ptr(mag),
                                  _ptr(ophase), _stream(stream)),
               "cordic_r2p16")
        return
    _check(lib().cordic_r2p(cfg.ref, n, _ptr(x), _ptr(y), _ptr(mag),
                            _ptr(ophase), _stream(stream)), "cordic_r2p")


def fm_demod_workspace(n):
    """cordic_fm_demod_workspace: bytes of device scratch an fm_demod call of
    n samples needs (16-byte aligned)"""
    return int(lib().cordic_fm_demod_workspace(n))


def fm_demod_info(cfg):
    """cordic_fm_demod_info: (fused, tile) -- whether 16-byte-aligned 32-bit
    arrays of this core run the fused kernel, and its tile in samples"""
    fused, tile = C.c_int32(0), C.c_int32(0)
    _check(lib().cordic_fm_demod_info(cfg.ref, C.byref(fused), C.byref(tile)),
           "cordic_fm_demod_info")
    return int(fused.value), int(tile.value)


def fm_demod16_info(cfg):
    """cordic_fm_demod16_info: (fused, tile) -- whether int16 arrays of this
    core (IW, OW, PW <= 16), at any alignment, run the fused kernel, and its
    tile in samples"""
    fused, tile = C.c_int32(0), C.c_int32(0)
    _check(lib().cordic_fm_demod16_info(cfg.ref, C.byref(fused),
                                        C.byref(tile)),
           "cordic_fm_demod16_info")
    return int(fused.value), int(tile.value)


def fm_demod(cfg, x, y, mag, freq, work, n=None, phase0=0, last=None,
             stream=None):
    """cordic_fm_demod: mag[i] as r2p, freq[i] = the converter's phase step
    from sample i-1 to i, sign extended from PW bits; the phase in front of
    sample 0 is phase0 + last[0] (mod 2^PW) and last (a one-word device
    tensor, optional) receives the phase of sample n-1.  int16 arrays select
    cordic_fm_demod16.  work: device scratch of fm_demod_workspace(n) bytes
    (16-byte aligned), the caller's."""
    n = x.numel() if n is None else n
    if work is None and n:
        raise TypeError("work: a device buffer of fm_demod_workspace(n) bytes")
    if hasattr(work, "numel") and hasattr(work, "element_size") \
            and work.numel() * work.element_size() < fm_demod_workspace(n):
        raise ValueError("work: %d bytes, fm_demod_workspace(%d) = %d"
                         % (work.numel() * work.element_size(), n,
                            fm_demod_workspace(n)))
    fn = "cordic_fm_demod"
    if any(_is16(t) for t in (x, y, mag, freq)):
        fn += "16"
        _same16(fn, x, y, mag, freq)
    _check(getattr(lib(), fn)(cfg.ref, n, _ptr(x), _ptr(y),
                              phase0 & 0xffffffff, _ptr(last), _ptr(mag),
                              _ptr(freq), _ptr(work), _stream(stream)), fn)


class _CDemodJob(C.Structure):
    """cordic_demod_job"""
    _fields_ = [("d_xval", C.c_void_p), ("d_yval", C.c_void_p),
                ("d_omag", C.c_void_p), ("d_ofreq", C.c_void_p),
                ("d_last", C.c_void_p), ("n", C.c_uint64),
                ("phase0", C.c_uint32), ("reserved", C.c_uint32)]


_DEMOD_KEYS = ("x", "y", "mag", "freq", "n", "phase0", "last")


class DemodBank:
    """cordic_demodbank: many fm_demod jobs of one r2p / sr2p core, cut once
    and run in at most two launches.  jobs: tuples (x, y, mag, freq, n, phase0,
    last) or dicts with those keys; x, y, mag, freq are int32 tensors or device
    addresses, last a one-word device tensor or None; n None: x.numel()."""

    _create = "cordic_demodbank_create"

    def __init__(self, cfg, jobs):
        jobs = [tuple(jb.get(k) for k in _DEMOD_KEYS) if isinstance(jb, dict)
                else tuple(jb) for jb in jobs]
        self._keep = jobs          # the tensors behind the addresses
        arr = (_CDemodJob * max(1, len(jobs)))()
        for k, (x, y, mag, freq, n, phase0, last) in enumerate(jobs):
            arr[k].d_xval = _ptr(x)
            arr[k].d_yval = _ptr(y)
            arr[k].d_omag = _ptr(mag)
            arr[k].d_ofreq = _ptr(freq)
            arr[k].d_last = _ptr(last)
            arr[k].n = x.numel() if n is None else n
            arr[k].phase0 = (phase0 or 0) & 0xffffffff
        h = C.c_void_p()
        _check(getattr(lib(), self._create)(cfg.ref, len(jobs), arr,
                                            C.byref(h)), self._create)
        self._h = h

    def info(self):
        a, b, c = C.c_uint64(), C.c_uint32(), C.c_uint32()
        d, e = C.c_int32(), C.c_int32()
        _check(lib().cordic_demodbank_info(self._h, C.byref(a), C.byref(b),
                                           C.byref(c), C.byref(d), C.byref(e)),
               "cordic_demodbank_info")
        return dict(samples=a.value, tiles=b.value, tail_jobs=c.value,
                    fused=d.value, tile=e.value)

    def run(self, stream=None):
        _check(lib().cordic_demodbank_run(self._h, _stream(stream)),
               "cordic_demodbank_run")

    def close(self):
        if getattr(self, "_h", None):
            lib().cordic_demodbank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DemodBank16(DemodBank):
    """cordic_demodbank_create16: a DemodBank of fm_demod16 jobs -- x, y, mag,
    freq are int16 tensors or device addresses (cordic_demod_job16 has the
    layout of cordic_demod_job); last stays a 32-bit word.  info, run and close
    are DemodBank's."""

    _create = "cordic_demodbank_create16"

    def __init__(self, cfg, jobs):
        for jb in jobs:
            jb = tuple(jb.get(k) for k in _DEMOD_KEYS) if isinstance(jb, dict) \
                else tuple(jb)
            _same16(self._create, *jb[0:4])
        DemodBank.__init__(self, cfg, jobs)


class _CFmMixJob(C.Structure):
    """cordic_fmmix_job"""
    _fields_ = [("d_fcw", C.c_void_p), ("d_pm", C.c_void_p),
                ("d_xval", C.c_void_p), ("d_yval", C.c_void_p),
                ("d_oxval", C.c_void_p), ("d_oyval", C.c_void_p),
                ("d_acc", C.c_void_p), ("n", C.c_uint64),
                ("phase0", C.c_uint32), ("reserved", C.c_uint32)]


_FMMIX_KEYS = ("fcw", "pm", "x", "y", "ox", "oy", "n", "phase0", "acc")
# a job key that is a tensor or a device address, and its field in the C struct
_JOB_FIELDS = {"fcw": "d_fcw", "pm": "d_pm", "x": "d_xval", "y": "d_yval",
               "ox": "d_oxval", "oy": "d_oyval", "iq": "d_iq", "oiq": "d_oiq",
               "mag": "d_omag",
               "freq": "d_ofreq", "acc": "d_acc", "last": "d_last"}


class _SpanBank:
    """What MixBank and RxBank share: info, run, close and __del__ on the
    handle self._h, through the C functions <_prefix>_info, _run and _destroy."""

    _prefix = None
    _keys = _job = _create = _create_decim = None

    def _open(self, plan, conv, jobs, log2r):
        """Packs `jobs` -- tuples in the order of self._keys, or dicts with
        those keys -- into an array of self._job (_JOB_FIELDS; n None:
        fcw.numel()) and creates the handle: <_create>(plan, *conv, njobs,
        jobs, &h), or <_create_decim> with log2r in front of njobs."""
        jobs = [tuple(jb.get(k) for k in self._keys) if isinstance(jb, dict)
                else tuple(jb) for jb in jobs]
        self._keep = (plan, jobs)   # the plan and the tensors behind the addresses
        arr = (self._job * max(1, len(jobs)))()
        for k, jb in enumerate(jobs):
            if len(jb) != len(self._keys):
                raise ValueError("a job is (%s)" % ", ".join(self._keys))
            for key, v in zip(self._keys, jb):
                if key == "n":
                    arr[k].n = jb[0].numel() if v is None else v
                elif key in _JOB_FIELDS:
                    setattr(arr[k], _JOB_FIELDS[key], _ptr(v))
                else:           # phase0, dphase0
                    setattr(arr[k], key, (v or 0) & 0xffffffff)
        h = C.c_void_p()
        name = self._create if log2r is None else self._create_decim
        _check(getattr(lib(), name)(
            getattr(plan, "_h", plan), *conv,
            *(() if log2r is None else (log2r,)), len(jobs), arr, C.byref(h)),
            name)
        self._h = h

    def info(self):
        a, b = C.c_uint64(), C.c_uint32()
        c, d = C.c_int32(), C.c_int32()
        name = self._prefix + "_info"
        _check(getattr(lib(), name)(self._h, C.byref(a), C.byref(b), C.byref(c),
                                    C.byref(d)), name)
        return dict(samples=a.value, spans=b.value, fused=c.value,
                    tile=d.value)

    def run(self, stream=None):
        name = self._prefix + "_run"
        _check(getattr(lib(), name)(self._h, _stream(stream)), name)

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self._prefix + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MixBank(_SpanBank):
    """cordic_mixbank: many fm_mix jobs of one p2r / sp2r plan, cut once and
    run in two launches.  jobs: tuples (fcw, pm, x, y, ox, oy, n, phase0, acc)
    or dicts with those keys; fcw, x, y, ox, oy are int32 tensors or device
    addresses, pm one more or None, acc a one-word device tensor or None; n
    None: fcw.numel().  The plan must stay open as long as the bank.
    log2r = k > 0 (cordic_mixbank_create_decim): a bank of fm_mix_decim jobs
    -- one k for the whole bank, every n a multiple of 2**k, ox and oy of
    n >> k elements."""

    _prefix = "cordic_mixbank"
    _create = "cordic_mixbank_create"
    _create_decim = "cordic_mixbank_create_decim"
    _keys, _job = _FMMIX_KEYS, _CFmMixJob

    def __init__(self, plan, jobs, log2r=None):
        self._open(plan, (), jobs, log2r)


class MixBank16(MixBank):
    """cordic_mixbank_create16: a MixBank of fm_mix16 jobs -- x, y, ox, oy are
    int16 tensors or device addresses (cordic_fmmix_job16 has the layout of
    cordic_fmmix_job); fcw, pm and acc stay 32-bit.  info, run and close are
    MixBank's."""

    _create = "cordic_mixbank_create16"
    _create_decim = "cordic_mixbank_create_decim16"

    def __init__(self, plan, jobs, log2r=None):
        for jb in jobs:
            jb = tuple(jb.get(k) for k in _FMMIX_KEYS) if isinstance(jb, dict) \
                else tuple(jb)
            _same16(self._create, *jb[2:6])
        MixBank.__init__(self, plan, jobs, log2r)


class _CFmMixJobC16(C.Structure):
    """cordic_fmmix_job_c16"""
    _fields_ = [("d_fcw", C.c_void_p), ("d_pm", C.c_void_p),
                ("d_iq", C.c_void_p), ("d_oiq", C.c_void_p),
                ("d_acc", C.c_void_p), ("n", C.c_uint64),
                ("phase0", C.c_uint32), ("reserved", C.c_uint32)]


_FMMIX_C16_KEYS = ("fcw", "pm", "iq", "oiq", "n", "phase0", "acc")


class MixBankC16(_SpanBank):
    """cordic_mixbank_create_c16: a MixBank of fm_mix_c16 jobs on INTERLEAVED
    int16 I/Q, in and out.  jobs: tuples (fcw, pm, iq, oiq, n, phase0, acc) or
    dicts with those keys; iq and oiq are int16 tensors (or device addresses)
    of 2 n and 2 (n >> log2r) shorts, I0 Q0 I1 Q1 ..; fcw, pm and acc stay
    32-bit; n None: fcw.numel().  log2r = k > 0
    (cordic_mixbank_create_decim_c16): a bank of fm_mix_decim_c16 jobs.  info,
    run and close are MixBank's: the handle is an ordinary cordic_mixbank."""

    _prefix = "cordic_mixbank"
    _create = "cordic_mixbank_create_c16"
    _create_decim = "cordic_mixbank_create_decim_c16"
    _keys, _job = _FMMIX_C16_KEYS, _CFmMixJobC16

    def __init__(self, plan, jobs, log2r=0):
        for jb in jobs:
            jb = tuple(jb.get(k) for k in _FMMIX_C16_KEYS) if isinstance(jb, dict) \
                else tuple(jb)
            _same16(self._create, *jb[2:4])
        self._open(plan, (), jobs, log2r or None)


class _CFmRxJob(C.Structure):
    """cordic_fmrx_job"""
    _fields_ = [("d_fcw", C.c_void_p), ("d_pm", C.c_void_p),
                ("d_xval", C.c_void_p), ("d_yval", C.c_void_p),
                ("d_omag", C.c_void_p), ("d_ofreq", C.c_void_p),
                ("d_acc", C.c_void_p), ("d_last", C.c_void_p),
                ("n", C.c_uint64), ("phase0", C.c_uint32),
                ("dphase0", C.c_uint32), ("reserved", C.c_uint64)]


_FMRX_KEYS = ("fcw", "pm", "x", "y", "mag", "freq", "n", "phase0", "acc",
              "dphase0", "last")


class RxBank(_SpanBank):
    """cordic_rxbank: many fm_rx jobs of one p2r / sp2r plan and one r2p /
    sr2p converter, cut once and run in two launches.  jobs: tuples (fcw, pm,
    x, y, mag, freq, n, phase0, acc, dphase0, last) or dicts with those keys;
    fcw, x, y, mag, freq are int32 tensors or device addresses, pm one more or
    None, acc and last one-word device tensors or None; n None: fcw.numel().
    The plan must stay open as long as the bank; conv is copied.
    log2r = k > 0 (cordic_rxbank_create_decim): a bank of fm_rx_decim jobs --
    one k for the whole bank, every n a multiple of 2**k, mag and freq of
    n >> k elements."""

    _prefix = "cordic_rxbank"
    _create = "cordic_rxbank_create"
    _create_decim = "cordic_rxbank_create_decim"
    _keys, _job = _FMRX_KEYS, _CFmRxJob

    def __init__(self, plan, conv, jobs, log2r=None):
        self._open(plan, (conv.ref if conv is not None else None,), jobs, log2r)


class RxBank16(RxBank):
    """cordic_rxbank_create16: an RxBank of fm_rx16 jobs -- x, y, mag, freq
    are int16 tensors or device addresses (cordic_fmrx_job16 has the layout of
    cordic_fmrx_job); fcw, pm, acc and last stay 32-bit.  info, run and close
    are RxBank's."""

    _create = "cordic_rxbank_create16"
    _create_decim = "cordic_rxbank_create_decim16"

    def __init__(self, plan, conv, jobs, log2r=None):
        for jb in jobs:
            jb = tuple(jb.get(k) for k in _FMRX_KEYS) if isinstance(jb, dict) \
                else tuple(jb)
            _same16(self._create, *jb[2:6])
        RxBank.__init__(self, plan, conv, jobs, log2r)


class _CFmRxJobC16(C.Structure):
    """cordic_fmrx_job_c16"""
    _fields_ = [("d_fcw", C.c_void_p), ("d_pm", C.c_void_p),
                ("d_iq", C.c_void_p),
                ("d_omag", C.c_void_p), ("d_ofreq", C.c_void_p),
                ("d_acc", C.c_void_p), ("d_last", C.c_void_p),
                ("n", C.c_uint64), ("phase0", C.c_uint32),
                ("dphase0", C.c_uint32), ("reserved", C.c_uint64)]


_FMRX_C16_KEYS = ("fcw", "pm", "iq", "mag", "freq", "n", "phase0", "acc",
                  "dphase0", "last")


class RxBankC16(_SpanBank):
    """cordic_rxbank_create_c16: an RxBank of fm_rx_c16 jobs on INTERLEAVED
    int16 I/Q.  jobs: tuples (fcw, pm, iq, mag, freq, n, phase0, acc, dphase0,
    last) or dicts with those keys; iq is an int16 tensor (or device address)
    of 2 n shorts, I0 Q0 I1 Q1 .., mag and freq int16 tensors; fcw, pm, acc and
    last stay 32-bit; n None: fcw.numel().  log2r = k > 0
    (cordic_rxbank_create_decim_c16): a bank of fm_rx_decim_c16 jobs.  info,
    run and close are RxBank's: the handle is an ordinary cordic_rxbank."""

    _prefix = "cordic_rxbank"
    _create = "cordic_rxbank_create_c16"
    _create_decim = "cordic_rxbank_create_decim_c16"
    _keys, _job = _FMRX_C16_KEYS, _CFmRxJobC16

    def __init__(self, plan, conv, jobs, log2r=None):
        for jb in jobs:
            jb = tuple(jb.get(k) for k in _FMRX_C16_KEYS) if isinstance(jb, dict) \
                else tuple(jb)
            _same16(self._create, *jb[2:5])
        self._open(plan, (conv.ref if conv is not None else None,), jobs, log2r)


class _CHostStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("chunks", C.c_int32),
                ("chunk_samples", C.c_int32), ("staged_inputs", C.c_int32),
                ("staged_outputs", C.c_int32), ("copy_threads", C.c_int32),
                ("seeded_plan", C.c_int32), ("lanes", C.c_int32),
                ("seconds", C.c_double)]


class HostArray:
    """n 32-bit words of PINNED host memory (cordic_host_alloc) as a numpy
    array: what the host-array entry points DMA in place."""

    def __init__(self, n, dtype="int32"):
        import weakref
        import numpy as np
        p = C.c_void_p()
        _check(lib().cordic_host_alloc(C.byref(p), max(1, n) * 4),
               "cordic_host_alloc")
        buf = (C.c_uint32 * max(1, n)).from_address(p.value)
        # the pinned block lives as long as ANY numpy view of it does (views
        # keep `buf` alive through their .base chain): it is released when the
        # ctypes buffer is collected, not when close() is called
        weakref.finalize(buf, lib().cordic_host_free, C.c_void_p(p.value))
        self.array = np.frombuffer(buf, dtype=np.uint32, count=n).view(dtype)

    def close(self):
        """drop this handle's reference (the memory goes once no view of
        `.array` is left)"""
        self.array = None


def host_last_stats():
    st = _CHostStats()
    _check(lib().cordic_host_last_stats(C.byref(st)), "cordic_host_last_stats")
    return {k: getattr(st, k) for k, _ in _CHostStats._fields_}


def host_release():
    lib().cordic_host_release()


def host_set_devices(devices):
    """device ordinals the host-array calls spread over ([] / None: the
    current device only)"""
    devices = list(devices or [])
    arr = (C.c_int * max(1, len(devices)))(*devices)
    _check(lib().cordic_host_set_devices(arr, len(devices)),
           "cordic_host_set_devices")


def host_lane_stats(lane):
    st = _CHostStats()
    _check(lib().cordic_host_lane_stats(lane, C.byref(st)),
           "cordic_host_lane_stats")
    return {k: getattr(st, k) for k, _ in _CHostStats._fields_}


def _host_out(out, n, dtypes, what):
    """caller-provided output arrays of a host-array call: the C pipeline
    writes n contiguous words through the raw pointer, so anything else than a
    writable C-contiguous array of exactly n 32-bit words is refused here"""
    import numpy as np
    if out is None:
        return tuple(np.empty(n, dtype=d) for d in dtypes)
    if len(out) != len(dtypes):
        raise ValueError("%s: out= wants %d arrays" % (what, len(dtypes)))
    for a in out:
        if (not isinstance(a, np.ndarray) or a.dtype.itemsize != 4
                or a.dtype.kind not in "iu" or a.ndim != 1 or a.size != n
                or not a.flags.c_contiguous or not a.flags.writeable):
            raise ValueError("%s: out= arrays must be writable, C-contiguous, "
                             "one-dimensional, 32-bit, %d elements" % (what, n))
    return tuple(out)


def p2r_host(cfg, x, y, phase, out=None):
    """cordic_p2r_host on numpy arrays (x, y scalars: constant vectors).
    out = (ox, oy): write into these int32 arrays (e.g. HostArray.array)."""
    import numpy as np
    phase = np.ascontiguousarray(phase, dtype=np.uint32)
    n = phase.size
    scalar = np.ndim(x) == 0
    if scalar:
        xa = np.array([x], dtype=np.int32)
        ya = np.array([y], dtype=np.int32)
    else:
        xa = np.ascontiguousarray(x, dtype=np.int32)
        ya = np.ascontiguousarray(y, dtype=np.int32)
        if xa.size != n or ya.size != n:
            raise ValueError("cordic_p2r_host: x, y and phase differ in length")
    ox, oy = _host_out(out, n, (np.int32, np.int32), "cordic_p2r_host")
    _check(lib().cordic_p2r_host(
        cfg.ref, n, xa.ctypes.data_as(_i32p), ya.ctypes.data_as(_i32p),
        1 if scalar else 0, phase.ctypes.data_as(_u32p),
        ox.ctypes.data_as(_i32p), oy.ctypes.data_as(_i32p)),
        "cordic_p2r_host")
    return ox, oy


def r2p_host(cfg, x, y, out=None):
    import numpy as np
    xa = np.ascontiguousarray(x, dtype=np.int32)
    ya = np.ascontiguousarray(y, dtype=np.int32)
    n = xa.size
    if ya.size != n:
        raise ValueError("cordic_r2p_host: x and y differ in length")
    mag, ph = _host_out(out, n, (np.int32, np.uint32), "cordic_r2p_host")
    _check(lib().cordic_r2p_host(
        cfg.ref, n, xa.ctypes.data_as(_i32p), ya.ctypes.data_as(_i32p),
        mag.ctypes.data_as(_i32p), ph.ctypes.data_as(_u32p)),
        "cordic_r2p_host")
    return mag, ph


def fill_phase_ramp(phase, index0, shift, n=None, stream=None):
    n = phase.numel() if n is None else n
    _check(lib().cordic_fill_phase_ramp(_ptr(phase), n, index0, shift,
                                        _stream(stream)),
           "cordic_fill_phase_ramp")


def fill_iq_ramp(x, y, index0, mulx, muly, bits, n=None, stream=None):
    n = x.numel() if n is None else n
    _check(lib().cordic_fill_iq_ramp(_ptr(x), _ptr(y), n, index0, mulx, muly,
                                     bits, _stream(stream)),
           "cordic_fill_iq_ramp")


def digest_u32(words, index0, digest, n=None, stream=None):
    """digest (int64 device tensor, 1 element) += digest of words."""
    n = words.numel() if n is None else n
    _check(lib().cordic_digest_u32(_ptr(words), n, index0, _ptr(digest),
                                   _stream(stream)), "cordic_digest_u32")

"""Host-side Python mirror of the reference's Evaluator interface over the sealhip C ABI.

The product path is `libsealhip.so` (hand-written HIP for gfx950 behind include/sealhip.h); this module
only binds it with ctypes and mirrors the names, argument meaning and error behaviour of
seal::Evaluator (native/src/seal/evaluator.h) so that tests read like the reference's own.
There is NO CPU fallback: if the library or a HIP device is missing, calls raise.

Error mapping (native/src/seal/c/defines.h:34-49 <-> evaluator.cpp exceptions):
  E_INVALIDARG -> ValueError (std::invalid_argument), COR_E_INVALIDOPERATION -> LogicError
  (std::logic_error), E_POINTER -> TypeError, E_OUTOFMEMORY -> MemoryError, E_UNEXPECTED -> RuntimeError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# SEALHIP_LIBRARY selects another build of the same HIP library (tools/ab_build.sh, the sanitizer build); there is no
# non-HIP implementation to select.
LIB_PATH = os.environ.get("SEALHIP_LIBRARY") or os.path.join(os.path.dirname(_HERE), "lib", "libsealhip.so")

S_OK = 0
E_POINTER = 0x80004003
E_INVALIDARG = 0x80070057
E_OUTOFMEMORY = 0x8007000E
E_UNEXPECTED = 0x8000FFFF
COR_E_INVALIDOPERATION = 0x80131509

SCHEME_BFV, SCHEME_CKKS = 1, 2
MODE_PARITY, MODE_STRICT = 0, 1
BASE_Q, BASE_BSK, BASE_KEY = 0, 1, 2


class LogicError(RuntimeError):
    """std::logic_error of the reference (unsupported operation for the scheme, host-only context, ...)."""


class Params(C.Structure):
    _fields_ = [
        ("scheme", C.c_uint32),
        ("log_n", C.c_uint32),
        ("n_key_moduli", C.c_uint32),
        ("n_special_primes", C.c_uint32),
        ("key_moduli", C.POINTER(C.c_uint64)),
        ("plain_modulus", C.c_uint64),
        ("mode", C.c_uint32),
        ("device", C.c_int32),
    ]


_lib = None

# every symbol include/sealhip.h declares: name -> argtypes (restype is always long unless noted)
_vp, _u32, _u64, _sz, _i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, C.c_int32


class PolyPlan(C.Structure):
    """sealhip_poly_plan (include/sealhip.h)"""
    _fields_ = [("d", _u32), ("m", _u32), ("g", _u32), ("inner_level", _u32), ("out_level", _u32), ("n_products", _u32),
                ("out_scale", C.c_double), ("temp_bytes_per_item", _u64)]


class DftStage(C.Structure):
    """sealhip_dft_stage (include/sealhip.h)"""
    _fields_ = [("s0", _u32), ("r", _u32), ("h0", _u32), ("level", _u32), ("n_baby", _u32), ("n_giant", _u32), ("folded", _u32),
                ("reserved", _u32), ("scale", C.c_double)]


class DftPlan(C.Structure):
    """sealhip_dft_plan (include/sealhip.h)"""
    _fields_ = [("direction", _u32), ("n_stages", _u32), ("in_level", _u32), ("out_level", _u32), ("needs_conjugation", _u32),
                ("n_key_steps", _u32), ("table_words", _u64), ("temp_bytes_per_item", _u64), ("stages", DftStage * 16)]


class EvalModPlan(C.Structure):
    """sealhip_evalmod_plan (include/sealhip.h)"""
    _fields_ = [("K", _u32), ("r", _u32), ("degree", _u32), ("n_baby", _u32), ("poly_level", _u32), ("out_level", _u32),
                ("n_products", _u32), ("reserved", _u32), ("poly_scale_out", C.c_double), ("scales", C.c_double * 9),
                ("temp_bytes_per_item", _u64)]


class BootstrapPlan(C.Structure):
    """sealhip_bootstrap_plan (include/sealhip.h)"""
    _fields_ = [("k_top", _u32), ("c2s_out_level", _u32), ("evalmod_out_level", _u32), ("out_level", _u32),
                ("needs_conjugation", _u32), ("n_key_steps", _u32), ("raise_scale", C.c_double), ("s2c_gain", C.c_double),
                ("table_words", _u64), ("temp_bytes_per_item", _u64), ("evalmod", EvalModPlan)]


class LintransPlan(C.Structure):
    """sealhip_lintrans_plan (include/sealhip.h)"""
    _fields_ = [("d", _u32), ("n_diagonals", _u32), ("n1", _u32), ("n_baby", _u32), ("n_giant", _u32), ("n_key_steps", _u32),
                ("table_words", _u64), ("temp_bytes_per_item", _u64)]


DFT_COEFFS_TO_SLOTS, DFT_SLOTS_TO_COEFFS = 0, 1

SYMBOLS = {
    "sealhip_last_error_string": None,
    "sealhip_num_devices": [C.POINTER(C.c_int32)],
    "sealhip_context_create": [C.POINTER(Params), C.POINTER(_vp)],
    "sealhip_context_destroy": [_vp],
    "sealhip_context_first_level": [_vp, C.POINTER(_u32)],
    "sealhip_context_bsk_size": [_vp, _u32, C.POINTER(_u32)],
    "sealhip_set_stream": [_vp, _vp],
    "sealhip_use_default_stream": [_vp],
    "sealhip_synchronize": [_vp],
    "sealhip_context_lane_count": [_vp, C.POINTER(_u32)],
    "sealhip_debug_ntt_handoff": [_vp, _u32, _i32],
    "sealhip_malloc": [_vp, _sz, C.POINTER(_vp)],
    "sealhip_free": [_vp, _vp],
    "sealhip_memcpy_h2d": [_vp, _vp, _vp, _sz],
    "sealhip_memcpy_d2h": [_vp, _vp, _vp, _sz],
    "sealhip_profile_enable": [_vp, _i32],
    "sealhip_profile_fetch": [_vp, C.c_char_p, _sz],
    "sealhip_debug_ntt_table": [_vp, _u32, _u32, _vp, _sz],
    "sealhip_debug_rns_constants": [_vp, _u32, _u32, _vp, _sz, C.POINTER(_sz)],
    "sealhip_debug_bfv_multiply_plan": [_vp, _u32, _u32, _u32, _i32, _vp],
    "sealhip_debug_behz_dot_split": [_vp, _u32, C.POINTER(C.c_int32)],
    "sealhip_debug_ks_split_last": [_vp, _u32, _sz, C.POINTER(C.c_int32)],
    "sealhip_debug_ntt_split_last": [_vp, _u32, _u32, _i32, _vp, _vp],
    "sealhip_ntt_negacyclic_harvey_lazy": [_vp, _vp, _sz, _u32, _u32],
    "sealhip_ntt_negacyclic_harvey": [_vp, _vp, _sz, _u32, _u32],
    "sealhip_inverse_ntt_negacyclic_harvey_lazy": [_vp, _vp, _sz, _u32, _u32],
    "sealhip_inverse_ntt_negacyclic_harvey": [_vp, _vp, _sz, _u32, _u32],
    "sealhip_dyadic_product_coeffmod": [_vp, _vp, _vp, _sz, _u32, _u32, _vp],
    "sealhip_multiply_poly_scalar_coeffmod": [_vp, _vp, _sz, _u32, _u32, _u64, _vp],
    "sealhip_add_poly_coeffmod": [_vp, _vp, _vp, _sz, _u32, _u32, _vp],
    "sealhip_sub_poly_coeffmod": [_vp, _vp, _vp, _sz, _u32, _u32, _vp],
    "sealhip_negate_poly_coeffmod": [_vp, _vp, _sz, _u32, _u32, _vp],
    "sealhip_fastbconv_m_tilde": [_vp, _u32, _vp, _sz, _vp],
    "sealhip_sm_mrq": [_vp, _u32, _vp, _sz, _vp],
    "sealhip_fast_floor": [_vp, _u32, _vp, _sz, _vp],
    "sealhip_fastbconv_sk": [_vp, _u32, _vp, _sz, _vp],
    "sealhip_divide_and_round_q_last_inplace": [_vp, _u32, _vp, _sz],
    "sealhip_divide_and_round_q_last_ntt_inplace": [_vp, _u32, _vp, _sz],
    "sealhip_galois_elt_from_step": [_vp, _i32, C.POINTER(_u32)],
    "sealhip_apply_galois": [_vp, _vp, _sz, _u32, _u32, _vp],
    "sealhip_apply_galois_ntt": [_vp, _vp, _sz, _u32, _u32, _vp],
    "sealhip_kswitch_key_load": [_vp, _vp, _u32, _i32, C.POINTER(_vp)],
    "sealhip_kswitch_key_destroy": [_vp, _vp],
    "sealhip_modup_rns": [_vp, _u32, _u32, _vp, _sz],
    "sealhip_rescale_special_rns_inplace": [_vp, _u32, _vp, _sz],
    "sealhip_switch_key_inplace": [_vp, _u32, _vp, _vp, _sz, _vp],
    "sealhip_switch_key_partial": [_vp, _u32, _vp, _sz, _vp, _u32, _u32, _vp],
    "sealhip_switch_key_finish": [_vp, _u32, _vp, _vp, _sz, _u32],
    "sealhip_kswitch_digits": [_vp, _u32, _vp],
    "sealhip_evaluator_multiply": [_vp, _u32, _vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_evaluator_square": [_vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_evaluator_relinearize": [_vp, _u32, _vp, _u32, _sz, C.POINTER(_vp), _u32],
    "sealhip_evaluator_multiply_many": [_vp, _u32, _vp, _u32, _sz, C.POINTER(_vp), _u32, _vp],
    "sealhip_evaluator_exponentiate": [_vp, _u32, _vp, _u64, _sz, C.POINTER(_vp), _u32, _vp],
    "sealhip_evaluator_multiply_host": [_vp, _u32, _vp, _u32, _vp, _u32, _sz, _vp, C.POINTER(_vp), _u32],
    "sealhip_evaluator_relinearize_host": [_vp, _u32, _vp, _u32, _sz, C.POINTER(_vp), _u32],
    "sealhip_evaluator_rotate_vector_host": [_vp, _u32, _vp, _sz, _i32, C.POINTER(_u32), C.POINTER(_vp), _u32],
    "sealhip_evaluator_mod_switch_to_next_host": [_vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_evaluator_rescale_to_next_host": [_vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_evaluator_mod_switch_to_next": [_vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_evaluator_rescale_to_next": [_vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_evaluator_mod_switch_to_next_strided": [_vp, _u32, _vp, _u32, _sz, _sz, _vp],
    "sealhip_evaluator_rescale_to_next_strided": [_vp, _u32, _vp, _u32, _sz, _sz, _vp],
    "sealhip_evaluator_apply_galois": [_vp, _u32, _vp, _sz, _u32, _vp],
    "sealhip_evaluator_transform_to_ntt": [_vp, _u32, _vp, _u32, _sz],
    "sealhip_evaluator_transform_from_ntt": [_vp, _u32, _vp, _u32, _sz],
    "sealhip_evaluator_negate": [_vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_evaluator_add": [_vp, _u32, _vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_evaluator_sub": [_vp, _u32, _vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_evaluator_multiply_plain_ntt": [_vp, _u32, _vp, _u32, _sz, _vp, _sz],
    "sealhip_evaluator_multiply_plain": [_vp, _u32, _vp, _u32, _sz, _vp, _sz],
    "sealhip_evaluator_transform_plain_to_ntt": [_vp, _u32, _vp, _sz, _sz, _sz, _vp],
    "sealhip_evaluator_mod_switch_plain_to": [_vp, _u32, _vp, _sz, _u32, _vp],
    "sealhip_is_transparent": [_vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_transparency_sink": [_vp, _vp, _sz],
    "sealhip_debug_butterfly_rate": [_vp, _u32, _u32, _vp],
    "sealhip_debug_chunk_log": [_vp, _vp, _sz, _vp],
    "sealhip_modulo_poly_coeffs_63": [_vp, _vp, _sz, _u32, _u32, _vp],
    "sealhip_evaluator_rotate_vector": [_vp, _u32, _vp, _sz, _i32, C.POINTER(_u32), C.POINTER(_vp), _u32],
    "sealhip_evaluator_apply_galois_many": [_vp, _u32, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, _vp],
    "sealhip_evaluator_rotate_vector_many": [_vp, _u32, _vp, _sz, C.POINTER(_i32), _u32, C.POINTER(_u32), C.POINTER(_vp), _u32,
                                             _vp],
    "sealhip_pack_lwes_galois_elts": [_vp, _sz, _i32, C.POINTER(_u32), _u32, C.POINTER(_u32)],
    "sealhip_evaluator_extract_lwe": [_vp, _u32, _vp, _sz, C.POINTER(_u32), _sz, _vp, _vp],
    "sealhip_evaluator_pack_lwes": [_vp, _u32, _vp, _vp, _sz, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, _i32, _i32, _vp],
    "sealhip_expand_galois_elts": [_vp, _sz, C.POINTER(_u32), _u32, C.POINTER(_u32)],
    "sealhip_evaluator_expand": [_vp, _u32, _vp, _sz, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, _i32, _vp],
    "sealhip_evaluator_dot_plain": [_vp, _u32, _vp, _u32, _u32, _sz, _vp, _u32, _vp],
    "sealhip_evaluator_apply_galois_dot_plain": [_vp, _u32, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, _vp, _u32, _vp],
    "sealhip_evaluator_rotate_vector_dot_plain": [_vp, _u32, _vp, _sz, C.POINTER(_i32), _u32, C.POINTER(_u32), C.POINTER(_vp),
                                                  _u32, _vp, _u32, _vp],
    "sealhip_evaluator_apply_galois_bsgs_plain": [_vp, _u32, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, C.POINTER(_u32),
                                                  C.POINTER(_vp), _u32, _vp, _vp],
    "sealhip_evaluator_rotate_vector_bsgs_plain": [_vp, _u32, _vp, _sz, C.POINTER(_i32), _u32, C.POINTER(_i32), _u32,
                                                   C.POINTER(_u32), C.POINTER(_vp), _u32, _vp, _vp],
    "sealhip_evaluator_dot_product_max_terms": [_vp, _u32, C.POINTER(C.c_uint64)],
    "sealhip_evaluator_dot_product": [_vp, _u32, C.POINTER(_vp), C.POINTER(_vp), _u32, _sz, C.POINTER(_vp), _u32, _vp],
    "sealhip_evaluator_linear_combination": [_vp, _u32, C.POINTER(_vp), _u32, _u32, _sz, _vp, _vp, _u32, _vp],
    "sealhip_evaluator_polynomial_plan_ckks": [_vp, _u32, C.c_double, C.POINTER(C.c_double), _u32, _u32, _u32, C.c_double, _vp,
                                               C.POINTER(_u64), C.POINTER(_u64)],
    "sealhip_evaluator_evaluate_polynomial_ckks": [_vp, _u32, _vp, _sz, C.c_double, C.POINTER(C.c_double), _u32, _u32, _u32,
                                                   C.c_double, C.POINTER(_vp), _u32, _vp, C.POINTER(_u32),
                                                   C.POINTER(C.c_double)],
    "sealhip_evaluator_linear_combination_levels": [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32), C.POINTER(_u32), _u32, _u32, _sz,
                                                    _vp, _vp, _u32, _vp],
    "sealhip_evaluator_evaluate_polynomial": [_vp, _u32, _vp, _sz, C.POINTER(C.c_uint64), _u32, _u32, C.POINTER(_vp), _u32, _vp],
    "sealhip_evaluator_relinearize_rescale": [_vp, _u32, _vp, _u32, _sz, _sz, C.POINTER(_vp), _u32, _vp],
    "sealhip_evaluator_dot_product_rescale": [_vp, _u32, C.POINTER(_vp), C.POINTER(_vp), _u32, _sz, C.POINTER(_vp), _u32, _vp],
    "sealhip_evaluator_apply_galois_dot_plain_rescale": [_vp, _u32, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, _vp, _u32,
                                                         _vp],
    "sealhip_evaluator_rotate_vector_dot_plain_rescale": [_vp, _u32, _vp, _sz, C.POINTER(_i32), _u32, C.POINTER(_u32),
                                                          C.POINTER(_vp), _u32, _vp, _u32, _vp],
    "sealhip_evaluator_apply_galois_bsgs_plain_rescale": [_vp, _u32, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32,
                                                          C.POINTER(_u32), C.POINTER(_vp), _u32, _vp, _vp],
    "sealhip_evaluator_rotate_vector_bsgs_plain_rescale": [_vp, _u32, _vp, _sz, C.POINTER(_i32), _u32, C.POINTER(_i32), _u32,
                                                           C.POINTER(_u32), C.POINTER(_vp), _u32, _vp, _vp],
    "sealhip_evaluator_dft_plan": [_vp, _u32, _u32, C.POINTER(_u32), _u32, C.POINTER(_u32), _vp, C.POINTER(_u32), _u32],
    "sealhip_dft_stage_steps": [_vp, _u32, _u32, C.POINTER(_u32), _u32, C.POINTER(_u32), _u32, C.POINTER(_i32), C.POINTER(_i32)],
    "sealhip_dft_stage_values": [_vp, _u32, _u32, C.POINTER(_u32), _u32, C.POINTER(_u32), C.c_double, _u32, _vp],
    "sealhip_dft_stage_values_host": [_vp, _u32, _u32, C.POINTER(_u32), _u32, C.POINTER(_u32), C.c_double, _u32, _vp],
    "sealhip_dft_tables_create": [_vp, _u32, _u32, C.POINTER(_u32), _u32, C.POINTER(_u32), C.c_double, C.POINTER(_vp)],
    "sealhip_dft_tables_destroy": [_vp],
    "sealhip_dft_tables_plan": [_vp, _vp],
    "sealhip_dft_tables_stage": [_vp, _u32, C.POINTER(_vp)],
    "sealhip_evaluator_coeffs_to_slots": [_vp, _vp, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, _vp, _vp],
    "sealhip_evaluator_slots_to_coeffs": [_vp, _vp, _vp, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, _vp],
    "sealhip_linear_transform_plan": [_vp, _u32, _vp, _u32, _vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_u32), _u32],
    "sealhip_linear_transform_diagonals": [_vp, _vp, _u32, _vp],
    "sealhip_linear_transform_values": [_vp, _vp, _u32, _vp, _u32, C.c_double, _vp],
    "sealhip_linear_transform_values_host": [_vp, _vp, _u32, _vp, _u32, C.c_double, _vp],
    "sealhip_linear_transform_create": [_vp, _vp, _u32, _u32, C.c_double, C.c_double, C.POINTER(_vp)],
    "sealhip_linear_transform_destroy": [_vp],
    "sealhip_linear_transform_tables_plan": [_vp, _vp, C.POINTER(C.c_double)],
    "sealhip_linear_transform_tables_steps": [_vp, C.POINTER(_i32), C.POINTER(_i32)],
    "sealhip_linear_transform_tables_plain": [_vp, C.POINTER(_vp)],
    "sealhip_evaluator_linear_transform": [_vp, _vp, _u32, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, _i32, _vp],
    "sealhip_evaluator_mod_raise": [_vp, _u32, _vp, _sz, _u32, _vp],
    "sealhip_evaluator_double_angle": [_vp, _u32, _vp, _sz, C.c_double, C.POINTER(_vp), _u32, _vp, C.POINTER(C.c_double)],
    "sealhip_evalmod_coeffs": [_u32, _u32, _u32, C.POINTER(C.c_double)],
    "sealhip_evaluator_evalmod_plan": [_vp, _u32, C.c_double, _u32, _u32, _u32, _u32, C.c_double, _vp],
    "sealhip_evaluator_eval_mod": [_vp, _u32, _vp, _sz, C.c_double, _u32, _u32, _u32, _u32, C.c_double, C.POINTER(_vp), _u32, _vp,
                                   C.POINTER(_u32), C.POINTER(C.c_double)],
    "sealhip_evaluator_bootstrap_plan": [_vp, _u32, C.POINTER(_u32), _u32, C.POINTER(_u32), C.POINTER(_u32), _u32, C.POINTER(_u32), _u32, _u32, _u32, _u32, _vp, C.POINTER(_u32), _u32],
    "sealhip_bootstrap_tables_create": [_vp, _u32, C.POINTER(_u32), _u32, C.POINTER(_u32), C.POINTER(_u32), _u32, C.POINTER(_u32), _u32, _u32, _u32, _u32, C.POINTER(_vp)],
    "sealhip_bootstrap_tables_destroy": [_vp],
    "sealhip_bootstrap_tables_plan": [_vp, _vp],
    "sealhip_evaluator_bootstrap": [_vp, _vp, _u32, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, C.POINTER(_vp), _u32, _vp],
    "sealhip_decryptor_dot_product_ct_sk": [_vp, _u32, _vp, _u32, _sz, _vp, _i32, _vp],
    "sealhip_decrypt_scale_and_round": [_vp, _u32, _vp, _sz, _vp],
    "sealhip_decryptor_invariant_noise_budget": [_vp, _u32, _vp, _u32, _sz, _vp, _vp],
    "sealhip_decryptor_decrypt": [_vp, _u32, _vp, _u32, _sz, _vp, _i32, _vp],
    "sealhip_encrypt_zero_symmetric": [_vp, _u32, _i32, _vp, _vp, _vp, _sz, _vp],
    "sealhip_encrypt_zero_asymmetric": [_vp, _u32, _i32, _vp, _vp, _vp, _sz, _vp],
    "sealhip_encryptor_encrypt": [_vp, _u32, _vp, _vp, _sz, _vp, _vp, _sz, _vp],
    "sealhip_encryptor_encrypt_symmetric": [_vp, _u32, _vp, _vp, _sz, _vp, _vp, _i32, _sz, _vp],
    "sealhip_multiply_add_plain_with_scaling_variant": [_vp, _u32, _vp, _sz, _vp, _u32, _sz, _i32],
    "sealhip_evaluator_add_plain": [_vp, _u32, _vp, _u32, _sz, _vp, _sz, _i32],
    "sealhip_context_using_batching": [_vp, C.POINTER(_i32)],
    "sealhip_batch_encode": [_vp, _vp, _sz, _sz, _vp],
    "sealhip_batch_decode": [_vp, _vp, _sz, _vp],
    "sealhip_batch_encode_int64": [_vp, _vp, _sz, _sz, _vp],
    "sealhip_batch_decode_int64": [_vp, _vp, _sz, _vp],
    "sealhip_context_set_parms_id": [_vp, _u32, _vp],
    "sealhip_ciphertext_peek": [_vp, _sz, _vp],
    "sealhip_ciphertext_load": [_vp, _vp, _sz, _vp, _vp, _sz],
    "sealhip_ciphertext_save_size": [_vp, _u32, _u32, C.POINTER(_sz)],
    "sealhip_ciphertext_save": [_vp, _vp, _vp, _vp, _sz, C.POINTER(_sz)],
    "sealhip_ciphertext_save_seeded": [_vp, _vp, _vp, _vp, _vp, _sz, C.POINTER(_sz)],
    "sealhip_is_data_valid_for": [_vp, _u32, _vp, _u32, _sz, _vp],
    "sealhip_ciphertext_resize": [_vp, _u32, _vp, _u32, _vp, _u32, _sz],
    "sealhip_kswitch_key_load_stream": [_vp, _vp, _sz, _u32, C.POINTER(_vp), C.POINTER(_u64)],
    "sealhip_expand_seed_host": [_vp, _u32, _vp, _vp],
    "sealhip_expand_seed": [_vp, _u32, _vp, _sz, _vp, _sz],
    "sealhip_debug_seed_slack": [_vp, C.c_int64],
    "sealhip_sample_polys": [_vp, _vp, _sz, _u32, _u32, _vp, _sz],
    "sealhip_sample_polys_host": [_vp, _vp, _sz, _u32, _u32, _vp, _sz],
    "sealhip_sample_polys_split": [_vp, _vp, _sz, _u32, _u32, _vp, _vp],
    "sealhip_debug_sample_map": [_vp, _vp, _sz, _i32, _vp],
    "sealhip_generate_secret_key": [_vp, _vp, _vp],
    "sealhip_sample_fixed_weight": [_vp, _vp, _sz, _u32, _vp, _sz],
    "sealhip_sample_fixed_weight_host": [_vp, _vp, _sz, _u32, _vp, _sz],
    "sealhip_debug_fixed_weight_map": [_vp, _vp, _sz, _u32, _vp],
    "sealhip_generate_sparse_secret_key": [_vp, _vp, _u32, _vp],
    "sealhip_generate_switching_keys": [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _i32, C.POINTER(_vp)],
    "sealhip_evaluator_switch_secret": [_vp, _u32, _vp, _sz, _vp, _vp],
    "sealhip_generate_rgsw": [_vp, _vp, _vp, _u32, _u32, _vp, _vp, C.POINTER(_vp)],
    "sealhip_rgsw_create": [_vp, _vp, _vp, C.POINTER(_vp)],
    "sealhip_rgsw_export": [_vp, _vp, C.POINTER(_vp)],
    "sealhip_rgsw_destroy": [_vp, _vp],
    "sealhip_evaluator_external_product": [_vp, _u32, _vp, _sz, _vp, _vp, _vp],
    "sealhip_evaluator_cmux": [_vp, _u32, _vp, _vp, _sz, _vp, _vp],
    "sealhip_evaluator_select": [_vp, _u32, _vp, _sz, _u32, C.POINTER(_vp), _vp],
    "sealhip_debug_ext_mac_plan": [_vp, _u32, _sz, C.POINTER(_i32)],
    "sealhip_evaluator_multiply_monomial": [_vp, _u32, _vp, _sz, _sz, _vp, _sz, _i32, _vp],
    "sealhip_lwe_mod_switch": [_vp, _vp, _vp, _sz, _i32, _u32, _vp],
    "sealhip_generate_blind_rotation_keys": [_vp, _vp, _vp, _u32, _i32, _u32, _vp, _vp, C.POINTER(_vp)],
    "sealhip_evaluator_blind_rotate": [_vp, _u32, _vp, _sz, _sz, _vp, _u32, C.POINTER(_vp), _vp],
    "sealhip_evaluator_bootstrap_encapsulated": [_vp, _vp, _u32, _vp, _sz, C.POINTER(_u32), C.POINTER(_vp), _u32, C.POINTER(_vp), _u32, _vp, _vp, _vp],
    "sealhip_memset_zero": [_vp, _vp, _sz],
    "sealhip_ciphertext_load_many": [_vp, _vp, _vp, _sz, _vp, _vp, _sz],
    "sealhip_host_register": [_vp, _vp, _sz],
    "sealhip_host_unregister": [_vp, _vp],
    "sealhip_debug_blake2xb": [_vp, _sz, _vp, _sz, _vp, _sz],
    "sealhip_kswitch_keys_save": [_vp, C.POINTER(_vp), _u32, _vp, _sz, C.POINTER(_sz)],
    "sealhip_kswitch_keys_save_seeded": [_vp, C.POINTER(_vp), _u32, _vp, _sz, C.POINTER(_sz)],
    "sealhip_generate_relin_keys": [_vp, _vp, _u32, _vp, _vp, _i32, C.POINTER(_vp)],
    "sealhip_generate_galois_keys": [_vp, _vp, _vp, _u32, _vp, _vp, _i32, C.POINTER(_vp)],
    "sealhip_graph_capture_begin": [_vp],
    "sealhip_graph_capture_end": [_vp, C.POINTER(_vp)],
    "sealhip_graph_launch": [_vp, _vp],
    "sealhip_graph_destroy": [_vp, _vp],
    "sealhip_ckks_encode": [_vp, _u32, _vp, _sz, _sz, C.c_double, _vp],
    "sealhip_ckks_decode": [_vp, _u32, _vp, _sz, C.c_double, _vp],
    "sealhip_ckks_encode_value": [_vp, _u32, C.c_double, C.c_double, _sz, _vp],
    "sealhip_ckks_encode_int64": [_vp, _u32, C.c_int64, _sz, _vp],
    "sealhip_pool_alloc": [_vp, _sz, C.POINTER(_vp)],
    "sealhip_pool_release": [_vp, _vp],
    "sealhip_pool_trim": [_vp],
    "sealhip_pool_stats": [_vp, _vp],
    "sealhip_memcpy_d2d": [_vp, _vp, _vp, _sz],
    "sealhip_transparency_note": [_vp, _u32, _vp, _u32, _sz],
}


class PoolStats(C.Structure):
    """struct sealhip_pool_stats"""
    _fields_ = [("bytes_in_use", C.c_uint64), ("bytes_cached", C.c_uint64), ("device_mallocs", C.c_uint64),
                ("device_frees", C.c_uint64), ("hits", C.c_uint64), ("misses", C.c_uint64), ("cross_lane_hits", C.c_uint64)]


class CiphertextInfo(C.Structure):
    """sealhip_ciphertext_info: what Ciphertext::save_members writes ahead of the words (ciphertext.cpp:170-188)"""
    _fields_ = [("parms_id", C.c_uint64 * 4), ("is_ntt_form", C.c_uint32), ("size", C.c_uint32),
                ("coeff_modulus_size", C.c_uint32), ("seeded", C.c_uint32), ("poly_modulus_degree", C.c_uint64),
                ("scale", C.c_double), ("data_words", C.c_uint64), ("total_bytes", C.c_uint64)]


def ciphertext_peek(raw):
    """Header + metadata of a serialized ciphertext (no context needed)"""
    info = CiphertextInfo()
    buf = (C.c_char * len(raw)).from_buffer_copy(raw)
    _check(lib().sealhip_ciphertext_peek(C.addressof(buf), len(raw), C.addressof(info)))
    return info


def lib():
    """Load libsealhip.so; fails loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libsealhip.so is missing (%s): build it with __graft_entry__.build() / make -C gemini-seal_amd; "
                "there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, argtypes in SYMBOLS.items():
            fn = getattr(L, name)
            if argtypes is None:
                fn.restype = C.c_char_p
                fn.argtypes = []
            else:
                fn.restype = C.c_long
                fn.argtypes = argtypes
        _lib = L
    return _lib


def _check(hr):
    hr &= 0xFFFFFFFF
    if hr == S_OK:
        return
    msg = lib().sealhip_last_error_string().decode("utf-8", "replace")
    if hr == E_INVALIDARG:
        raise ValueError(msg)
    if hr == COR_E_INVALIDOPERATION:
        raise LogicError(msg)
    if hr == E_POINTER:
        raise TypeError(msg)
    if hr == E_OUTOFMEMORY:
        raise MemoryError(msg)
    raise RuntimeError("sealhip error 0x%08x: %s" % (hr, msg))


def num_devices():
    n = C.c_int32(0)
    _check(lib().sealhip_num_devices(C.byref(n)))
    return n.value


def _ptr(x):
    """Device pointer of a DeviceBuffer, a torch CUDA tensor, or a raw integer address."""
    if isinstance(x, DeviceBuffer):
        return x.ptr
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


class DeviceBuffer:
    """uint64 words in HBM, owned through sealhip_malloc / sealhip_free."""

    def __init__(self, ctx, words):
        self.ctx, self.words = ctx, int(words)
        p = C.c_void_p()
        _check(lib().sealhip_malloc(ctx.handle, self.words * 8, C.byref(p)))
        self.ptr = p.value

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        assert host.size == self.words, (host.size, self.words)
        _check(lib().sealhip_memcpy_h2d(self.ctx.handle, self.ptr, host.ctypes.data, host.size * 8))
        return self

    def download(self, shape=None):
        self.ctx.synchronize()  # also surfaces asynchronous kernel-side failures
        out = np.empty(self.words, dtype=np.uint64)
        _check(lib().sealhip_memcpy_d2h(self.ctx.handle, out.ctypes.data, self.ptr, self.words * 8))
        return out.reshape(shape) if shape is not None else out

    def free(self):
        if self.ptr:
            _check(lib().sealhip_free(self.ctx.handle, self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PoolBuffer(DeviceBuffer):
    """uint64 words in a block of the context's pool (sealhip_pool_alloc); free() releases it to the pool, stream-ordered
    on the calling thread's lane"""

    def __init__(self, ctx, words):
        self.ctx, self.words = ctx, int(words)
        p = C.c_void_p()
        _check(lib().sealhip_pool_alloc(ctx.handle, self.words * 8, C.byref(p)))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            ptr, self.ptr = self.ptr, None
            _check(lib().sealhip_pool_release(self.ctx.handle, ptr))


class KSwitchKeys:
    """One key-switch key (n_digits x 2 x n_key x N, keygenerator.cpp:325-369) resident in HBM."""

    def __init__(self, ctx, key, n_digits=None, from_host=True):
        self.ctx = ctx
        if from_host:
            key = np.ascontiguousarray(key, dtype=np.uint64)
            if n_digits is None:
                n_digits = key.shape[0]
            src = key.ctypes.data
        else:
            src = _ptr(key)
        h = C.c_void_p()
        _check(lib().sealhip_kswitch_key_load(ctx.handle, src, n_digits, 1 if from_host else 0, C.byref(h)))
        self.handle = h.value

    @classmethod
    def from_stream(cls, ctx, raw, index):
        """KSwitchKeys::load (kswitchkeys.cpp:87-150): keys_[index] of a serialized RelinKeys / GaloisKeys object, its digits
        copied straight from the byte stream into HBM. Returns None when the slot is empty."""
        buf = (C.c_char * len(raw)).from_buffer_copy(raw)
        h, slots = C.c_void_p(), _u64(0)
        _check(lib().sealhip_kswitch_key_load_stream(ctx.handle, C.addressof(buf), len(raw), index, C.byref(h), C.byref(slots)))
        if not h.value:
            return None
        self = cls.__new__(cls)
        self.ctx, self.handle, self.n_slots = ctx, h.value, slots.value
        return self

    @classmethod
    def _adopt(cls, ctx, handle):
        self = cls.__new__(cls)
        self.ctx, self.handle = ctx, handle
        return self

    def __del__(self):
        try:
            if self.handle:
                lib().sealhip_kswitch_key_destroy(self.ctx.handle, self.handle)
                self.handle = None
        except Exception:
            pass


class Rgsw:
    """One RGSW ciphertext: the key-switch keys K_b (new key m) and K_a (new key m s) in one device
    block. Made by Context.generate_rgsw or Context.rgsw_create."""

    @classmethod
    def _adopt(cls, ctx, handle):
        self = cls.__new__(cls)
        self.ctx, self.handle = ctx, handle
        return self

    def __del__(self):
        try:
            if self.handle:
                lib().sealhip_rgsw_destroy(self.ctx.handle, self.handle)
                self.handle = None
        except Exception:
            pass


def lut_test_vector(f, t, n):
    """The test vector of a lookup table for blind rotation: the plaintext coefficients
    tv[j] = f(floor(j t / 2N)), j < N, as int64. Messages are restricted to [0, t/2); with b_offset = N / t in
    Context.lwe_mod_switch the windows are centred, and the constant coefficient of X^(-phi~) tv is f(m)."""
    return np.array([f((j * t) // (2 * n)) for j in range(n)], dtype=np.int64)


def blake2xb(outlen, data, key=b""):
    """BLAKE2Xb of csrc/blake2xb.cpp (the PRNG under Ciphertext::expand_seed)"""
    out = C.create_string_buffer(outlen)
    _check(lib().sealhip_debug_blake2xb(out, outlen, data, len(data), key if key else None, len(key)))
    return out.raw


def save_kswitch_keys(ctx, keys, seeded=False):
    """KSwitchKeys::save (kswitchkeys.cpp:43-85): keys = list of KSwitchKeys or None (unused slot) -> the reference's byte
    stream, digit words copied straight from HBM. seeded: the Serializable<> form (sealhip_kswitch_keys_save_seeded: c_0
    and the seed of c_1 per digit) of keys generated with keep_seeds"""
    fn = lib().sealhip_kswitch_keys_save_seeded if seeded else lib().sealhip_kswitch_keys_save
    arr = (C.c_void_p * max(1, len(keys)))(*[(k.handle if k is not None else None) for k in keys])
    need = _sz(0)
    _check(fn(ctx.handle, arr, len(keys), None, 0, C.byref(need)))
    buf = (C.c_char * need.value)()
    written = _sz(0)
    _check(fn(ctx.handle, arr, len(keys), C.addressof(buf), need.value, C.byref(written)))
    return bytes(buf[: written.value])


def save_kswitch_keys_seeded(ctx, keys):
    """Serializable<RelinKeys / GaloisKeys>::save of generated keys (sealhip_kswitch_keys_save_seeded)"""
    return save_kswitch_keys(ctx, keys, seeded=True)


class Graph:
    """An instantiated hipGraph of engine launches (sealhip_graph)."""

    def __init__(self, ctx, handle):
        self.ctx, self.handle = ctx, handle

    def launch(self):
        _check(lib().sealhip_graph_launch(self.ctx.handle, self.handle))

    def __del__(self):
        try:
            if self.handle:
                lib().sealhip_graph_destroy(self.ctx.handle, self.handle)
                self.handle = None
        except Exception:
            pass


class Context:
    """Plain mirror of what the path needs from SEALContext (context.cpp:455-540)."""

    def __init__(self, scheme, log_n, key_moduli, n_special_primes=1, plain_modulus=0, mode=MODE_PARITY, device=0):
        self.scheme, self.log_n, self.n = scheme, log_n, 1 << log_n
        self.key_moduli = [int(x) for x in key_moduli]
        self.n_key, self.nsp = len(self.key_moduli), n_special_primes
        arr = (C.c_uint64 * self.n_key)(*self.key_moduli)
        p = Params(scheme, log_n, self.n_key, n_special_primes, arr, plain_modulus, mode, device)
        h = C.c_void_p()
        _check(lib().sealhip_context_create(C.byref(p), C.byref(h)))
        self.handle = h.value
        self.k_first = self.n_key - n_special_primes

    # -- memory
    def alloc(self, words):
        return DeviceBuffer(self, words)

    def upload(self, host):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        return DeviceBuffer(self, host.size).upload(host)

    def upload_i32(self, host):
        """small signed samples (int32) -> device; returns a DeviceBuffer holding the raw words"""
        host = np.ascontiguousarray(host, dtype=np.int32)
        assert host.size % 2 == 0
        return DeviceBuffer(self, host.size // 2).upload(host.view(np.uint64))

    def synchronize(self):
        _check(lib().sealhip_synchronize(self.handle))

    # -- pooled device memory (include/sealhip.h, sealhip_pool_*)
    def pool_alloc(self, words):
        """a PoolBuffer of `words` uint64 words; its free() releases the block to the pool"""
        return PoolBuffer(self, words)

    def pool_release(self, ptr):
        _check(lib().sealhip_pool_release(self.handle, _ptr(ptr)))

    def pool_trim(self):
        _check(lib().sealhip_pool_trim(self.handle))

    def pool_stats(self):
        """{bytes_in_use, bytes_cached, device_mallocs, device_frees, hits, misses, cross_lane_hits}"""
        st = PoolStats()
        _check(lib().sealhip_pool_stats(self.handle, C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in PoolStats._fields_}

    def memcpy_d2d(self, dst, src, words):
        """stream-ordered device-to-device copy of `words` uint64 words"""
        _check(lib().sealhip_memcpy_d2d(self.handle, _ptr(dst), _ptr(src), int(words) * 8))

    def transparency_note(self, k, ct, size, count):
        """the transparency read pass over `count` ciphertexts into the installed sink (sealhip_transparency_note)"""
        _check(lib().sealhip_transparency_note(self.handle, k, _ptr(ct), size, count))

    def set_stream(self, stream_ptr):
        """hipStream_t of the calling thread's lane (None/0: back to a private stream)"""
        _check(lib().sealhip_set_stream(self.handle, stream_ptr))

    def lane_count(self):
        v = C.c_uint32()
        _check(lib().sealhip_context_lane_count(self.handle, C.byref(v)))
        return v.value

    def use_default_stream(self):
        _check(lib().sealhip_use_default_stream(self.handle))

    def debug_ntt_handoff(self, spin_limit=0, suppress_signal=False):
        _check(lib().sealhip_debug_ntt_handoff(self.handle, spin_limit, 1 if suppress_signal else 0))

    def bsk_size(self, k):
        v = C.c_uint32()
        _check(lib().sealhip_context_bsk_size(self.handle, k, C.byref(v)))
        return v.value

    def rows(self, k, base):
        if base == BASE_Q:
            return k
        if base == BASE_BSK:
            return self.bsk_size(k)
        return k + self.nsp

    def profile_enable(self, on=True):
        _check(lib().sealhip_profile_enable(self.handle, 1 if on else 0))

    def profile_fetch(self):
        """{kernel tag: {"launches", "ms", "units"}} from HIP events on the launch stream; clears the records."""
        import json

        buf = C.create_string_buffer(1 << 16)
        _check(lib().sealhip_profile_fetch(self.handle, buf, len(buf)))
        return json.loads(buf.value.decode())

    # -- introspection (host only)
    def debug_ntt_table(self, prime_index, kind):
        out = np.empty(self.n, dtype=np.uint64)
        _check(lib().sealhip_debug_ntt_table(self.handle, prime_index, kind, out.ctypes.data, out.size))
        return out

    def debug_rns_constants(self, k, which):
        out = np.empty(70 * 70, dtype=np.uint64)
        w = C.c_size_t()
        _check(lib().sealhip_debug_rns_constants(self.handle, k, which, out.ctypes.data, out.size, C.byref(w)))
        return out[: w.value].copy()

    BFV_PLAN_FIELDS = ("k", "B", "nB", "square", "redc_small", "gather", "defer", "fused_tensor", "tensor_apx", "lift_top",
                       "lift_kernel", "floor_kernel", "deferred_top")

    def debug_bfv_multiply_plan(self, k, size_a=2, size_b=2, square=False):
        """{field: int} -- the dispatch of a BFV multiply (square: of one size-2 operand) at level k
        (sealhip_debug_bfv_multiply_plan; instance 1..15 exact k, 32 run-time k, 64 step-by-step)"""
        out = np.zeros(len(self.BFV_PLAN_FIELDS), dtype=np.int32)
        _check(lib().sealhip_debug_bfv_multiply_plan(self.handle, k, size_a, size_b, 1 if square else 0, out.ctypes.data))
        return dict(zip(self.BFV_PLAN_FIELDS, (int(x) for x in out)))

    def debug_behz_dot_split(self, k):
        """30 or 31: the split position of the exact-k BEHZ kernels' dot products at level k (sealhip_debug_behz_dot_split)"""
        v = C.c_int32()
        _check(lib().sealhip_debug_behz_dot_split(self.handle, k, C.byref(v)))
        return v.value

    def debug_ks_split_last(self, k, count):
        """True where a key switch of a chunk of `count` items at level k stores its digit rows without the forward transform's
        last layer and the inner product's pair form applies it (sealhip_debug_ks_split_last)"""
        v = C.c_int32()
        _check(lib().sealhip_debug_ks_split_last(self.handle, k, count, C.byref(v)))
        return bool(v.value)

    def debug_ntt_split_last(self, prime_index, src, dst, treatment=0, exact=False):
        """one forward transform without its last layer of the N words of `src` on key prime prime_index, into `dst` as E | O
        (sealhip_debug_ntt_split_last)"""
        _check(lib().sealhip_debug_ntt_split_last(self.handle, prime_index, treatment, 1 if exact else 0, _ptr(src), _ptr(dst)))

    def galois_elt_from_step(self, step):
        v = C.c_uint32()
        _check(lib().sealhip_galois_elt_from_step(self.handle, step, C.byref(v)))
        return v.value

    # -- L2 functions (names of native/src/seal/util/*.h)
    def pack_lwes_galois_elts(self, n, trace=False):
        """the Galois elements 2^t + 1 that Evaluator.pack_lwes of n samples needs, ascending (works on host-only contexts)"""
        count = _u32(0)
        _check(lib().sealhip_pack_lwes_galois_elts(self.handle, n, 1 if trace else 0, None, 0, C.byref(count)))
        elts = (_u32 * max(1, count.value))()
        _check(lib().sealhip_pack_lwes_galois_elts(self.handle, n, 1 if trace else 0, elts, count.value, C.byref(count)))
        return [int(elts[i]) for i in range(count.value)]

    def expand_galois_elts(self, n):
        """the Galois elements N / 2^(t-1) + 1 that Evaluator.expand into n ciphertexts needs, ascending (works on host-only
        contexts)"""
        count = _u32(0)
        _check(lib().sealhip_expand_galois_elts(self.handle, n, None, 0, C.byref(count)))
        elts = (_u32 * max(1, count.value))()
        _check(lib().sealhip_expand_galois_elts(self.handle, n, elts, count.value, C.byref(count)))
        return [int(elts[i]) for i in range(count.value)]

    def ntt_negacyclic_harvey_lazy(self, data, count, k, base=BASE_Q):
        _check(lib().sealhip_ntt_negacyclic_harvey_lazy(self.handle, _ptr(data), count, k, base))

    def ntt_negacyclic_harvey(self, data, count, k, base=BASE_Q):
        _check(lib().sealhip_ntt_negacyclic_harvey(self.handle, _ptr(data), count, k, base))

    def inverse_ntt_negacyclic_harvey_lazy(self, data, count, k, base=BASE_Q):
        _check(lib().sealhip_inverse_ntt_negacyclic_harvey_lazy(self.handle, _ptr(data), count, k, base))

    def inverse_ntt_negacyclic_harvey(self, data, count, k, base=BASE_Q):
        _check(lib().sealhip_inverse_ntt_negacyclic_harvey(self.handle, _ptr(data), count, k, base))

    def dyadic_product_coeffmod(self, a, b, count, k, result, base=BASE_Q):
        _check(lib().sealhip_dyadic_product_coeffmod(self.handle, _ptr(a), _ptr(b), count, k, base, _ptr(result)))

    def multiply_poly_scalar_coeffmod(self, a, count, k, scalar, result, base=BASE_Q):
        _check(lib().sealhip_multiply_poly_scalar_coeffmod(self.handle, _ptr(a), count, k, base, scalar, _ptr(result)))

    def add_poly_coeffmod(self, a, b, count, k, result, base=BASE_Q):
        _check(lib().sealhip_add_poly_coeffmod(self.handle, _ptr(a), _ptr(b), count, k, base, _ptr(result)))

    def sub_poly_coeffmod(self, a, b, count, k, result, base=BASE_Q):
        _check(lib().sealhip_sub_poly_coeffmod(self.handle, _ptr(a), _ptr(b), count, k, base, _ptr(result)))

    def modulo_poly_coeffs_63(self, a, count, k, result, base=BASE_Q):
        _check(lib().sealhip_modulo_poly_coeffs_63(self.handle, _ptr(a), count, k, base, _ptr(result)))

    def is_transparent(self, ct, size, k, count):
        """Ciphertext::is_transparent (ciphertext.h:471-476) for each ciphertext of the batch -> numpy bool array"""
        flags = np.zeros(count, dtype=np.uint8)
        _check(lib().sealhip_is_transparent(self.handle, k, _ptr(ct), size, count, flags.ctypes.data))
        return flags.astype(bool)

    def transparency_sink(self, flags, capacity):
        """The is_transparent test as a flag output of the Evaluator operations: `flags` = device buffer of `capacity`
        uint32 words (None removes the sink); after an operation flags[i] != 0 iff polynomials 1.. of result i are non-zero."""
        _check(lib().sealhip_transparency_sink(self.handle, _ptr(flags) if flags is not None else None, capacity))

    def dot_product_ct_sk(self, ct, size, k, count, sk_powers_ntt, is_ntt_form, out):
        """Decryptor::dot_product_ct_sk_array (decryptor.cpp:218-265)"""
        _check(lib().sealhip_decryptor_dot_product_ct_sk(self.handle, k, _ptr(ct), size, count, _ptr(sk_powers_ntt),
                                                         1 if is_ntt_form else 0, _ptr(out)))

    def decrypt_scale_and_round(self, k, poly, count, out):
        """RNSTool::decrypt_scale_and_round (rns.cpp:1070-1126)"""
        _check(lib().sealhip_decrypt_scale_and_round(self.handle, k, _ptr(poly), count, _ptr(out)))

    def invariant_noise_budget(self, ct, size, k, count, sk_powers_ntt):
        """Decryptor::invariant_noise_budget (decryptor.cpp:269-325) per BFV ciphertext of the batch -> numpy int32 array"""
        budgets = np.zeros(max(1, count), dtype=np.int32)
        _check(lib().sealhip_decryptor_invariant_noise_budget(self.handle, k, _ptr(ct), size, count, _ptr(sk_powers_ntt),
                                                              budgets.ctypes.data))
        return budgets[:count]

    def decrypt(self, ct, size, k, count, sk_powers_ntt, is_ntt_form, plain):
        """Decryptor::decrypt (decryptor.cpp:51-150): BFV plain[count][N] mod t, CKKS plain[count][k][N] (NTT form)"""
        _check(lib().sealhip_decryptor_decrypt(self.handle, k, _ptr(ct), size, count, _ptr(sk_powers_ntt),
                                               1 if is_ntt_form else 0, _ptr(plain)))

    # ---- encrypt-side arithmetic (the random samples come from the caller)
    def encrypt_zero_symmetric(self, rows, is_ntt_form, a_ntt, noise, sk_ntt, count, ct):
        """util::encrypt_zero_symmetric (util/rlwe.cpp:204-300); noise = int32 device words (count x N)"""
        _check(lib().sealhip_encrypt_zero_symmetric(self.handle, rows, 1 if is_ntt_form else 0, _ptr(a_ntt), _ptr(noise),
                                                    _ptr(sk_ntt), count, _ptr(ct)))

    # ---- Encryptor (encryptor.cpp:106-259) with the samples handed in
    def encrypt(self, k, pk_ntt, plain, u, noise, count, ct, plain_item_stride=None):
        """Encryptor::encrypt / encrypt_zero(parms_id) with a public key: ct[count][2][k][N] (device). pk_ntt: 2 x n_key x N
        (NTT form); plain: None (encrypt_zero), BFV count x N < t at the first level, CKKS count x k x N in NTT form;
        plain_item_stride: words between plaintexts (None: back to back, 0: one for all); u: count x N, noise: count x 2 x N
        int32 (device, e.g. upload_i32)"""
        if plain_item_stride is None:
            plain_item_stride = self.n if self.scheme == SCHEME_BFV else k * self.n
        _check(lib().sealhip_encryptor_encrypt(self.handle, k, _ptr(pk_ntt), _ptr(plain) if plain is not None else None,
                                               plain_item_stride, _ptr(u), _ptr(noise), count, _ptr(ct)))

    def encrypt_symmetric(self, k, sk_ntt, plain, seeds, noise, count, ct, save_seed=False, plain_item_stride=None):
        """Encryptor::encrypt_symmetric / encrypt_zero_symmetric: c_1 expanded on the device from seeds (count x 8 words,
        host), sk_ntt: n_key x N (NTT form), noise: count x N int32 (device). save_seed: the reference's seeded branch
        (BFV: a sampled in coefficient form; dropped when k x N < 9). ct receives both polynomials."""
        if plain_item_stride is None:
            plain_item_stride = self.n if self.scheme == SCHEME_BFV else k * self.n
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        _check(lib().sealhip_encryptor_encrypt_symmetric(self.handle, k, _ptr(sk_ntt),
                                                         _ptr(plain) if plain is not None else None, plain_item_stride,
                                                         seeds.ctypes.data, _ptr(noise), 1 if save_seed else 0, count,
                                                         _ptr(ct)))

    def save_seeded(self, info, src, seed_words):
        """Serializable<Ciphertext>::save of a seeded encryption (ciphertext.cpp:189-208): c_0 from src, then the seed"""
        seed = np.ascontiguousarray(np.array([int(x) for x in seed_words], dtype=np.uint64))
        need = _sz(0)
        _check(lib().sealhip_ciphertext_save_seeded(self.handle, C.addressof(info), _ptr(src), seed.ctypes.data, None, 0,
                                                    C.byref(need)))
        buf = (C.c_char * need.value)()
        written = _sz(0)
        _check(lib().sealhip_ciphertext_save_seeded(self.handle, C.addressof(info), _ptr(src), seed.ctypes.data,
                                                    C.addressof(buf), need.value, C.byref(written)))
        return bytes(buf[: written.value])

    def encrypt_zero_asymmetric(self, rows, is_ntt_form, pk_ntt, u, noise, count, ct):
        """util::encrypt_zero_asymmetric (util/rlwe.cpp:140-202); u = count x N, noise = count x 2 x N int32"""
        _check(lib().sealhip_encrypt_zero_asymmetric(self.handle, rows, 1 if is_ntt_form else 0, _ptr(pk_ntt), _ptr(u),
                                                     _ptr(noise), count, _ptr(ct)))

    def multiply_add_plain_with_scaling_variant(self, k, plain, ct, size, count, plain_stride=None, subtract=False):
        """util/scalingvariant.cpp:15-92 on c_0 of every ciphertext"""
        stride = self.n if plain_stride is None else plain_stride
        _check(lib().sealhip_multiply_add_plain_with_scaling_variant(self.handle, k, _ptr(plain), stride, _ptr(ct), size,
                                                                     count, 1 if subtract else 0))

    def ckks_encode(self, values, k, scale, plain=None):
        """CKKSEncoder::encode (ckks.h:405-617): values = numpy complex array [count][n_values] -> device plaintexts
        [count][k][N] (NTT form)"""
        values = np.ascontiguousarray(values, dtype=np.complex128)
        count, nv = values.shape
        dv = DeviceBuffer(self, values.size * 2).upload(values.view(np.uint64))
        if plain is None:
            plain = self.alloc(count * k * self.n)
        _check(lib().sealhip_ckks_encode(self.handle, k, _ptr(dv), nv, count, float(scale), _ptr(plain)))
        self.synchronize()
        dv.free()
        return plain

    def ckks_encode_value(self, value, k, scale, count=1, plain=None):
        """CKKSEncoder::encode(double value, ...) (ckks.cpp:80-216); an int value takes the int64 overload (:218-275)"""
        if plain is None:
            plain = self.alloc(count * k * self.n)
        if isinstance(value, (int, np.integer)):
            _check(lib().sealhip_ckks_encode_int64(self.handle, k, int(value), count, _ptr(plain)))
        else:
            _check(lib().sealhip_ckks_encode_value(self.handle, k, float(value), float(scale), count, _ptr(plain)))
        return plain

    def ckks_decode(self, plain, k, count, scale):
        """CKKSEncoder::decode (ckks.h:623-747) -> numpy complex array [count][N/2]"""
        out = self.alloc(count * self.n)
        _check(lib().sealhip_ckks_decode(self.handle, k, _ptr(plain), count, float(scale), _ptr(out)))
        res = out.download().view(np.complex128).reshape(count, self.n // 2)
        out.free()
        return res

    # ---- HIP graphs: capture a fixed sequence of operations on fixed buffers, replay it as one launch
    def capture(self, fn):
        """Runs fn() once eagerly (allocations, tables), then captures a second run from the context's stream."""
        fn()
        self.synchronize()
        _check(lib().sealhip_graph_capture_begin(self.handle))
        try:
            fn()
        finally:
            h = C.c_void_p()
            hr = lib().sealhip_graph_capture_end(self.handle, C.byref(h))
        _check(hr)
        return Graph(self, h.value)

    # ---- ciphertext wire format
    def set_parms_id(self, k, parms_id):
        arr = (C.c_uint64 * 4)(*[int(x) for x in parms_id])
        _check(lib().sealhip_context_set_parms_id(self.handle, k, C.addressof(arr)))

    def expand_seed(self, rows, seed_words):
        """Ciphertext::expand_seed (ciphertext.cpp:126-133) on the host: rows x N words of c_1"""
        seed = np.array([int(x) for x in seed_words], dtype=np.uint64)
        out = np.zeros((rows, self.n), dtype=np.uint64)
        _check(lib().sealhip_expand_seed_host(self.handle, rows, seed.ctypes.data, out.ctypes.data))
        return out

    def load_ciphertext(self, raw, dst, capacity_words=None):
        """Ciphertext::load (ciphertext.cpp:228-330): words go from `raw` (host bytes) straight into dst (device)"""
        info = CiphertextInfo()
        buf = (C.c_char * len(raw)).from_buffer_copy(raw)
        cap = dst.words if capacity_words is None else capacity_words
        _check(lib().sealhip_ciphertext_load(self.handle, C.addressof(buf), len(raw), C.addressof(info), _ptr(dst), cap))
        return info

    def expand_seeds(self, rows, seeds, out, item_stride=0):
        """Ciphertext::expand_seed on the device (sealhip_expand_seed): seeds = count x 8 words; out + i * item_stride
        (0: rows x N) receives the rows x N words of c_1 for seed i"""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 8))
        _check(lib().sealhip_expand_seed(self.handle, rows, seeds.ctypes.data, seeds.shape[0], _ptr(out), item_stride))

    # ---- KeyGenerator (keygenerator.cpp:146-240, :325-369) with the samples handed in
    def generate_relin_keys(self, sk_ntt, count, seeds, noise, keep_seeds=False):
        """KeyGenerator::relin_keys(count, save_seed): keys for sk^2 .. sk^(count+1). sk_ntt: n_key x N (device); seeds:
        count x d x 8 words (host); noise: count x d x N int32 (device, e.g. upload_i32). Returns count KSwitchKeys."""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        out = (C.c_void_p * max(1, count))()
        _check(lib().sealhip_generate_relin_keys(self.handle, _ptr(sk_ntt), count, seeds.ctypes.data if seeds.size else None,
                                                 _ptr(noise) if noise is not None else None, 1 if keep_seeds else 0, out))
        return [KSwitchKeys._adopt(self, out[i]) for i in range(count)]

    def generate_galois_keys(self, sk_ntt, galois_elts, seeds, noise, keep_seeds=False):
        """KeyGenerator::galois_keys(galois_elts, save_seed) without the duplicate skipping (distinct elements only): key i is
        for apply_galois_ntt(sk, galois_elts[i]). Layouts as generate_relin_keys. Returns one KSwitchKeys per element."""
        elts = np.ascontiguousarray(np.asarray(galois_elts, dtype=np.uint32).reshape(-1))
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        out = (C.c_void_p * max(1, elts.size))()
        _check(lib().sealhip_generate_galois_keys(self.handle, _ptr(sk_ntt), elts.ctypes.data if elts.size else None, elts.size,
                                                  seeds.ctypes.data if seeds.size else None,
                                                  _ptr(noise) if noise is not None else None, 1 if keep_seeds else 0, out))
        return [KSwitchKeys._adopt(self, out[i]) for i in range(elts.size)]

    # ---- RLWE samples from seeds
    def sample_polys(self, seeds, n_ternary, n_noise, out, item_stride=0):
        """sealhip_sample_polys: seeds = count x 8 words (host); out + i * item_stride int32 words (0: (n_ternary + n_noise)
        x N) receives item i's n_ternary ternary and then n_noise noise polynomials of N int32 values (device)"""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 8))
        _check(lib().sealhip_sample_polys(self.handle, seeds.ctypes.data, seeds.shape[0], n_ternary, n_noise, _ptr(out),
                                          item_stride))

    def sample_polys_split(self, seeds, n_ternary, n_noise, ternary, noise):
        """sealhip_sample_polys_split: the same samples as ternary[count][n_ternary][N] and noise[count][n_noise][N]"""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 8))
        _check(lib().sealhip_sample_polys_split(self.handle, seeds.ctypes.data, seeds.shape[0], n_ternary, n_noise,
                                                _ptr(ternary) if ternary is not None else None,
                                                _ptr(noise) if noise is not None else None))

    def sample_polys_host(self, seeds, n_ternary, n_noise, item_stride=0):
        """sealhip_sample_polys_host: the same words computed on the host; returns int32 [count][item_stride or polys x N]"""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 8))
        width = item_stride if item_stride else (n_ternary + n_noise) * self.n
        out = np.zeros((seeds.shape[0], width), dtype=np.int32)
        _check(lib().sealhip_sample_polys_host(self.handle, seeds.ctypes.data, seeds.shape[0], n_ternary, n_noise,
                                               out.ctypes.data, item_stride))
        return out

    def debug_sample_map(self, words, kind):
        """sealhip_debug_sample_map: the kernels' map (kind 0 ternary, 1 noise) of the given 64-bit words; returns int32"""
        words = np.ascontiguousarray(np.asarray(words, dtype=np.uint64).reshape(-1))
        n = words.size
        src = self.upload(words if n else np.zeros(1, dtype=np.uint64))
        dst = self.alloc((n + 1) // 2 + 1)
        _check(lib().sealhip_debug_sample_map(self.handle, _ptr(src), n, kind, _ptr(dst)))
        return dst.download().view(np.int32)[:n].copy()

    def generate_secret_key(self, seed, out=None):
        """sealhip_generate_secret_key: the n_key x N words (NTT form, device) of the secret key drawn from `seed` (8 words)"""
        seed = np.ascontiguousarray(np.asarray(seed, dtype=np.uint64).reshape(8))
        out = self.alloc(self.n_key * self.n) if out is None else out
        _check(lib().sealhip_generate_secret_key(self.handle, seed.ctypes.data, _ptr(out)))
        return out

    # ---- fixed-weight secrets
    def sample_fixed_weight(self, seeds, h, out, item_stride=0):
        """sealhip_sample_fixed_weight: seeds = count x 8 words (host); out + i * item_stride int32 words (0: N) receives the
        N coefficients of weight exactly h for seed i (device): the h smallest of the seed's first N stream words are the
        support, bit 0 of a word the sign"""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 8))
        _check(lib().sealhip_sample_fixed_weight(self.handle, seeds.ctypes.data, seeds.shape[0], h, _ptr(out), item_stride))

    def sample_fixed_weight_host(self, seeds, h, item_stride=0):
        """sealhip_sample_fixed_weight_host: the same words computed on the host; returns int32 [count][item_stride or N]"""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 8))
        out = np.zeros((seeds.shape[0], item_stride if item_stride else self.n), dtype=np.int32)
        _check(lib().sealhip_sample_fixed_weight_host(self.handle, seeds.ctypes.data, seeds.shape[0], h, out.ctypes.data,
                                                      item_stride))
        return out

    def debug_fixed_weight_map(self, words, h):
        """sealhip_debug_fixed_weight_map: the rank kernel on the given 64-bit words [n_polys][N]; returns int32 of that shape"""
        words = np.ascontiguousarray(np.asarray(words, dtype=np.uint64).reshape(-1, self.n))
        src = self.upload(words)
        dst = self.alloc((words.size + 1) // 2)
        _check(lib().sealhip_debug_fixed_weight_map(self.handle, _ptr(src), words.shape[0], h, _ptr(dst)))
        return dst.download().view(np.int32)[: words.size].reshape(words.shape).copy()

    def generate_sparse_secret_key(self, seed, h, out=None):
        """sealhip_generate_sparse_secret_key: generate_secret_key with the fixed-weight polynomial of weight h"""
        seed = np.ascontiguousarray(np.asarray(seed, dtype=np.uint64).reshape(8))
        out = self.alloc(self.n_key * self.n) if out is None else out
        _check(lib().sealhip_generate_sparse_secret_key(self.handle, seed.ctypes.data, h, _ptr(out)))
        return out

    def generate_switching_keys(self, sk_to_ntt, sk_from_ntt, n_keys, level, seeds, noise, keep_seeds=False):
        """sealhip_generate_switching_keys: key i switches what is encrypted under sk_from_ntt[i] (n_keys x n_key x N,
        device) to sk_to_ntt. level = n_ct: the full key; a smaller level: a key for key switches at levels <= level only
        (encapsulation's dense -> sparse key takes level 1). Layouts as generate_relin_keys. Returns n_keys KSwitchKeys."""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        out = (C.c_void_p * max(1, n_keys))()
        _check(lib().sealhip_generate_switching_keys(self.handle, _ptr(sk_to_ntt),
                                                     _ptr(sk_from_ntt) if sk_from_ntt is not None else None, n_keys, level,
                                                     seeds.ctypes.data if seeds.size else None,
                                                     _ptr(noise) if noise is not None else None, 1 if keep_seeds else 0, out))
        return [KSwitchKeys._adopt(self, out[i]) for i in range(n_keys)]

    def generate_rgsw(self, sk_ntt, m_coeff, n, level, seeds, noise):
        """sealhip_generate_rgsw: n Rgsw objects from m_coeff (n x N int32, device, small signed coefficients). seeds: n x 2
        x digits x 8 words (host), noise: n x 2 x digits x N int32 (device); half h of message i uses [i][h]. level as
        generate_switching_keys."""
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        out = (C.c_void_p * max(1, n))()
        _check(lib().sealhip_generate_rgsw(self.handle, _ptr(sk_ntt), _ptr(m_coeff) if m_coeff is not None else None, n, level,
                                           seeds.ctypes.data if seeds.size else None,
                                           _ptr(noise) if noise is not None else None, out))
        return [Rgsw._adopt(self, out[i]) for i in range(n)]

    def rgsw_create(self, key_b, key_a):
        """sealhip_rgsw_create: the Rgsw whose halves are copies of two KSwitchKeys (K_b: new key m, K_a: new key m s)"""
        h = C.c_void_p()
        _check(lib().sealhip_rgsw_create(self.handle, key_b.handle, key_a.handle, C.byref(h)))
        return Rgsw._adopt(self, h.value)

    def rgsw_export(self, rgsw):
        """sealhip_rgsw_export: (K_b, K_a) as two owned KSwitchKeys holding copies of the halves"""
        out = (C.c_void_p * 2)()
        _check(lib().sealhip_rgsw_export(self.handle, rgsw.handle, out))
        return KSwitchKeys._adopt(self, out[0]), KSwitchKeys._adopt(self, out[1])

    def debug_ext_mac_plan(self, k, count):
        """what the external product's inner product would run for a chunk of `count` items at level k
        (sealhip_debug_ext_mac_plan): dict(family "loop" | "items", nd2, split, group)"""
        out = (_i32 * 4)()
        _check(lib().sealhip_debug_ext_mac_plan(self.handle, k, count, out))
        return dict(family={1: "loop", 2: "items"}.get(out[0], "refused"), nd2=out[1], split=bool(out[2]), group=out[3])

    def upload_u32(self, host):
        """uint32 words (exponents) -> device; an odd count is padded with one zero word"""
        host = np.ascontiguousarray(host, dtype=np.uint32).reshape(-1)
        if host.size % 2:
            host = np.concatenate([host, np.zeros(1, dtype=np.uint32)])
        return DeviceBuffer(self, host.size // 2).upload(host.view(np.uint64))

    def lwe_mod_switch(self, lwe_a, lwe_b, n_samples, ternary, b_offset, exps_out):
        """sealhip_lwe_mod_switch: level-1 samples lwe_a (n x 1 x N) and lwe_b (n x 1) to the exponent
        rows of Evaluator.blind_rotate, n x (1 + N) uint32 for a binary secret and n x (1 + 2N) for a ternary one"""
        _check(lib().sealhip_lwe_mod_switch(self.handle, _ptr(lwe_a), _ptr(lwe_b), n_samples, 1 if ternary else 0, b_offset,
                                            _ptr(exps_out)))

    def generate_blind_rotation_keys(self, sk_ntt, lwe_secret, n_lwe, ternary, level, seeds, noise):
        """sealhip_generate_blind_rotation_keys: the n_steps = n_lwe (binary) or 2 n_lwe (ternary) Rgsw encryptions of the
        indicators [s_j = 1] (and [s_j = -1]) of lwe_secret (n_lwe int32, device). seeds: n_steps x 2 x digits x 8 words (host),
        noise: n_steps x 2 x digits x N int32 (device), as generate_rgsw takes them."""
        n = n_lwe * (2 if ternary else 1)
        seeds = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1))
        out = (C.c_void_p * max(1, n))()
        _check(lib().sealhip_generate_blind_rotation_keys(self.handle, _ptr(sk_ntt), _ptr(lwe_secret) if lwe_secret is not None else None,
                                                          n_lwe, 1 if ternary else 0, level, seeds.ctypes.data if seeds.size else None,
                                                          _ptr(noise) if noise is not None else None, out))
        return [Rgsw._adopt(self, out[i]) for i in range(n)]

    def memset_zero(self, buf, nbytes):
        """stream-ordered zero fill of device memory (sealhip_memset_zero)"""
        _check(lib().sealhip_memset_zero(self.handle, _ptr(buf), nbytes))

    def debug_seed_slack(self, extra):
        """candidates provisioned per seed beyond rows x N on this thread's lane (< 0: the default; sealhip_debug_seed_slack)"""
        _check(lib().sealhip_debug_seed_slack(self.handle, int(extra)))

    def load_ciphertexts(self, raws, dst, item_stride):
        """Ciphertext::load for a batch (sealhip_ciphertext_load_many): stream i lands at dst + i * item_stride words;
        returns the list of CiphertextInfo"""
        n = len(raws)
        bufs = [(C.c_char * max(1, len(r))).from_buffer_copy(r) if r else (C.c_char * 1)() for r in raws]
        ptrs = (C.c_void_p * max(1, n))(*[C.addressof(b) for b in bufs])
        lens = (C.c_size_t * max(1, n))(*[len(r) for r in raws])
        infos = (CiphertextInfo * max(1, n))()
        _check(lib().sealhip_ciphertext_load_many(self.handle, C.addressof(ptrs), C.addressof(lens), n, C.addressof(infos),
                                                  _ptr(dst), item_stride))
        return [infos[i] for i in range(n)]

    def save_ciphertext(self, info, src):
        """Ciphertext::save (ciphertext.cpp:170-226), uncompressed -> bytes"""
        need = _sz(0)
        _check(lib().sealhip_ciphertext_save_size(self.handle, info.size, info.coeff_modulus_size, C.byref(need)))
        buf = (C.c_char * need.value)()
        written = _sz(0)
        _check(lib().sealhip_ciphertext_save(self.handle, C.addressof(info), _ptr(src), C.addressof(buf), need.value,
                                             C.byref(written)))
        return bytes(buf[: written.value])

    def is_data_valid_for(self, ct, size, k, count):
        """is_data_valid_for (valcheck.cpp:284-317) per ciphertext of the batch -> numpy bool array"""
        flags = np.zeros(count, dtype=np.uint8)
        _check(lib().sealhip_is_data_valid_for(self.handle, k, _ptr(ct), size, count, flags.ctypes.data))
        return flags.astype(bool)

    # ---- BatchEncoder
    @property
    def using_batching(self):
        flag = _i32(0)
        _check(lib().sealhip_context_using_batching(self.handle, C.byref(flag)))
        return bool(flag.value)

    def batch_encode(self, values, n_values, count, plain):
        """BatchEncoder::encode (batchencoder.cpp:113-154)"""
        _check(lib().sealhip_batch_encode(self.handle, _ptr(values), n_values, count, _ptr(plain)))

    def batch_decode(self, plain, count, values):
        """BatchEncoder::decode (batchencoder.cpp:339-376)"""
        _check(lib().sealhip_batch_decode(self.handle, _ptr(plain), count, _ptr(values)))

    def batch_encode_int64(self, values, n_values, count, plain):
        """BatchEncoder::encode(vector<int64_t>) (batchencoder.cpp:156-198); values = device words holding int64"""
        _check(lib().sealhip_batch_encode_int64(self.handle, _ptr(values), n_values, count, _ptr(plain)))

    def batch_decode_int64(self, plain, count, values):
        """BatchEncoder::decode(vector<int64_t>) (batchencoder.cpp:378-420)"""
        _check(lib().sealhip_batch_decode_int64(self.handle, _ptr(plain), count, _ptr(values)))

    def negate_poly_coeffmod(self, a, count, k, result, base=BASE_Q):
        _check(lib().sealhip_negate_poly_coeffmod(self.handle, _ptr(a), count, k, base, _ptr(result)))

    def fastbconv_m_tilde(self, k, inp, count, out):
        _check(lib().sealhip_fastbconv_m_tilde(self.handle, k, _ptr(inp), count, _ptr(out)))

    def sm_mrq(self, k, inp, count, out):
        _check(lib().sealhip_sm_mrq(self.handle, k, _ptr(inp), count, _ptr(out)))

    def fast_floor(self, k, inp, count, out):
        _check(lib().sealhip_fast_floor(self.handle, k, _ptr(inp), count, _ptr(out)))

    def fastbconv_sk(self, k, inp, count, out):
        _check(lib().sealhip_fastbconv_sk(self.handle, k, _ptr(inp), count, _ptr(out)))

    def divide_and_round_q_last_inplace(self, k, data, count):
        _check(lib().sealhip_divide_and_round_q_last_inplace(self.handle, k, _ptr(data), count))

    def divide_and_round_q_last_ntt_inplace(self, k, data, count):
        _check(lib().sealhip_divide_and_round_q_last_ntt_inplace(self.handle, k, _ptr(data), count))

    def apply_galois(self, inp, count, k, galois_elt, out):
        _check(lib().sealhip_apply_galois(self.handle, _ptr(inp), count, k, galois_elt, _ptr(out)))

    def apply_galois_ntt(self, inp, count, k, galois_elt, out):
        _check(lib().sealhip_apply_galois_ntt(self.handle, _ptr(inp), count, k, galois_elt, _ptr(out)))

    def modup_rns(self, k, src_bundle_index, ext, count):
        _check(lib().sealhip_modup_rns(self.handle, k, src_bundle_index, _ptr(ext), count))

    def rescale_special_rns_inplace(self, k, poly, count):
        _check(lib().sealhip_rescale_special_rns_inplace(self.handle, k, _ptr(poly), count))

    def switch_key_inplace(self, k, ct, target, count, key):
        _check(lib().sealhip_switch_key_inplace(self.handle, k, _ptr(ct), _ptr(target), count, key.handle))

    # ---- SURVEY 8(e) latency mode: the digits of one key switch split across devices
    def kswitch_digits(self, k):
        d = C.c_uint32()
        _check(lib().sealhip_kswitch_digits(self.handle, k, C.byref(d)))
        return d.value

    def chunk_log(self):
        """[(batch size, items per arena chunk), ...] of this thread's last operations (sealhip_debug_chunk_log); clears it"""
        buf = (C.c_size_t * 128)()
        n = C.c_size_t(0)
        _check(lib().sealhip_debug_chunk_log(self.handle, buf, 64, C.byref(n)))
        return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n.value)]

    def butterfly_rate(self, kind, prime_index=0):
        """butterflies per second of one butterfly sequence on this device (sealhip_debug_butterfly_rate)"""
        d = C.c_double(0.0)
        _check(lib().sealhip_debug_butterfly_rate(self.handle, kind, prime_index, C.byref(d)))
        return d.value

    def switch_key_partial(self, k, target, count, key, digit_begin, digit_end, partial):
        """inner product of evaluator.cpp:2302-2349 over the digits [digit_begin, digit_end) -> count x 2 x (k+nsp) x N"""
        _check(lib().sealhip_switch_key_partial(self.handle, k, _ptr(target), count, key.handle, digit_begin, digit_end,
                                                _ptr(partial)))

    def switch_key_finish(self, k, ct, partial_sum, count, n_partials):
        """the rest of the key switch (evaluator.cpp:2351-2366) on the element-wise sum of n_partials devices' partials"""
        _check(lib().sealhip_switch_key_finish(self.handle, k, _ptr(ct), _ptr(partial_sum), count, n_partials))

    def close(self):
        if getattr(self, "handle", None):
            lib().sealhip_context_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Evaluator:
    """Batched mirror of seal::Evaluator for the hot path (native/src/seal/evaluator.h:246-1239).

    Ciphertexts are device buffers in the reference layout (size x k x N uint64), `count` of them back to back;
    `k` names the level (number of coefficient-modulus primes)."""

    def __init__(self, context):
        self.ctx = context

    def multiply(self, a, size_a, b, size_b, k, count, out):
        _check(lib().sealhip_evaluator_multiply(self.ctx.handle, k, _ptr(a), size_a, _ptr(b), size_b, count, _ptr(out)))

    def square(self, a, size_a, k, count, out):
        _check(lib().sealhip_evaluator_square(self.ctx.handle, k, _ptr(a), size_a, count, _ptr(out)))

    def relinearize_inplace(self, ct, size, k, count, relin_keys):
        keys = (C.c_void_p * max(1, len(relin_keys)))(*[rk.handle for rk in relin_keys])
        _check(lib().sealhip_evaluator_relinearize(self.ctx.handle, k, _ptr(ct), size, count, keys, len(relin_keys)))

    def mod_switch_to_next(self, ct, size, k, count, out, item_stride=0):
        """item_stride (words): the ciphertexts of `ct` sit that far apart (e.g. the size-2 result of relinearize inside its
        size-3 product); 0 = back to back"""
        if item_stride:
            _check(lib().sealhip_evaluator_mod_switch_to_next_strided(self.ctx.handle, k, _ptr(ct), size, item_stride, count,
                                                                     _ptr(out)))
        else:
            _check(lib().sealhip_evaluator_mod_switch_to_next(self.ctx.handle, k, _ptr(ct), size, count, _ptr(out)))

    def rescale_to_next(self, ct, size, k, count, out, item_stride=0):
        if item_stride:
            _check(lib().sealhip_evaluator_rescale_to_next_strided(self.ctx.handle, k, _ptr(ct), size, item_stride, count,
                                                                  _ptr(out)))
        else:
            _check(lib().sealhip_evaluator_rescale_to_next(self.ctx.handle, k, _ptr(ct), size, count, _ptr(out)))

    def apply_galois_inplace(self, ct, k, count, galois_elt, galois_key):
        _check(lib().sealhip_evaluator_apply_galois(self.ctx.handle, k, _ptr(ct), count, galois_elt, galois_key.handle))

    def rotate_vector_inplace(self, ct, k, count, steps, galois_keys):
        """rotate_internal (evaluator.cpp:1945-2000): direct key if present, else the NAF decomposition.
        galois_keys: dict galois_elt -> KSwitchKeys."""
        if steps == 0:
            return
        elt = self.ctx.galois_elt_from_step(steps)
        if elt in galois_keys:
            return self.apply_galois_inplace(ct, k, count, elt, galois_keys[elt])
        naf = _naf(steps)
        if len(naf) == 1:
            raise ValueError("Galois key not present")
        for s in naf:
            if abs(s) != (self.ctx.n >> 1):
                self.rotate_vector_inplace(ct, k, count, s, galois_keys)

    rotate_rows_inplace = rotate_vector_inplace

    def rotate_vector_native(self, ct, k, count, steps, galois_keys):
        """The same rotate_internal logic behind the C ABI (sealhip_evaluator_rotate_vector)."""
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(lib().sealhip_evaluator_rotate_vector(self.ctx.handle, k, _ptr(ct), count, steps, ea, ka, n_keys))

    def apply_galois_many(self, ct, k, count, elts, keys, out):
        """Hoisted rotation (sealhip_evaluator_apply_galois_many): `count` size-2 ciphertexts under every Galois element of
        `elts` with one decomposition of c_1; keys[i] is the KSwitchKeys of elts[i]. out: len(elts) x count x 2 x k x N,
        element-major; ct is not modified. Not the words of repeated apply_galois_inplace."""
        elts = [int(g) for g in elts]
        ea = (_u32 * max(1, len(elts)))(*elts)
        ka = (_vp * max(1, len(elts)))(*[key.handle for key in keys])
        _check(lib().sealhip_evaluator_apply_galois_many(self.ctx.handle, k, _ptr(ct), count, ea, ka, len(elts), _ptr(out)))

    def rotate_vector_many(self, ct, k, count, steps, galois_keys, out):
        """The same by rotation steps (sealhip_evaluator_rotate_vector_many): out: len(steps) x count x 2 x k x N; step 0
        copies the input, a step without its key in galois_keys (dict galois_elt -> KSwitchKeys) raises ValueError."""
        steps = [int(st) for st in steps]
        sa = (_i32 * max(1, len(steps)))(*steps)
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(lib().sealhip_evaluator_rotate_vector_many(self.ctx.handle, k, _ptr(ct), count, sa, len(steps), ea, ka, n_keys,
                                                          _ptr(out)))

    def extract_lwe(self, ct, k, count, indices, lwe_a, lwe_b):
        """Ring packing (sealhip_evaluator_extract_lwe): the LWE samples of the coefficients `indices`
        (host integers below N, any order, repeats allowed) of `count` size-2 ciphertexts in the scheme's form.
        lwe_a: count x len(indices) x k x N, lwe_b: count x len(indices) x k; ct is not modified."""
        idx = [int(i) for i in indices]
        _check(lib().sealhip_evaluator_extract_lwe(self.ctx.handle, k, _ptr(ct), count, _u32_array(idx), len(idx), _ptr(lwe_a),
                                                   _ptr(lwe_b)))

    def pack_lwes(self, lwe_a, lwe_b, k, n, count, galois_keys, out, trace=False, normalize=False):
        """sealhip_evaluator_pack_lwes: the n = 2^l samples of every item packed into one ciphertext, sample j at coefficient
        (N / n) j, times n (N with `trace`, which also clears every other coefficient; 1 with `normalize`). galois_keys: dict
        galois_elt -> KSwitchKeys with the elements of Context.pack_lwes_galois_elts(n, trace). out: count x 2 x k x N."""
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(lib().sealhip_evaluator_pack_lwes(self.ctx.handle, k, _ptr(lwe_a), _ptr(lwe_b), n, count, ea, ka, n_keys,
                                                 1 if trace else 0, 1 if normalize else 0, _ptr(out)))

    def expand(self, ct, k, count, n, galois_keys, out, normalize=False):
        """Oblivious expansion (sealhip_evaluator_expand): every one of `count` size-2 ciphertexts in the
        scheme's form into n = 2^l, output i holding n times coefficient i of the phase (1 times with `normalize`).
        galois_keys: dict galois_elt -> KSwitchKeys with the elements of Context.expand_galois_elts(n). out: count x n x 2 x
        k x N; ct is not modified."""
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(lib().sealhip_evaluator_expand(self.ctx.handle, k, _ptr(ct), count, n, ea, ka, n_keys, 1 if normalize else 0,
                                              _ptr(out)))

    def external_product(self, ct, k, count, rgsw, out, base=None):
        """out = base + ct (x) rgsw (sealhip_evaluator_external_product): count size-2 ciphertexts in the
        scheme's form against one Rgsw; base (count x 2 x k x N) None means zero. The phase is multiplied by the Rgsw's m."""
        _check(lib().sealhip_evaluator_external_product(self.ctx.handle, k, _ptr(ct), count, rgsw.handle,
                                                        _ptr(base) if base is not None else None, _ptr(out)))

    def cmux(self, ct0, ct1, k, count, rgsw, out):
        """out = ct0 + (ct1 - ct0) (x) rgsw (sealhip_evaluator_cmux): ct1 where the Rgsw encrypts 1, ct0 where it encrypts 0"""
        _check(lib().sealhip_evaluator_cmux(self.ctx.handle, k, _ptr(ct0), _ptr(ct1), count, rgsw.handle, _ptr(out)))

    def select(self, cts, k, count, rgsw_bits, out):
        """out[i] = cts[i][index] (sealhip_evaluator_select): cts count x 2^l x 2 x k x N, rgsw_bits the l Rgsw encryptions of
        the index's bits, least significant first; a CMux tree of l levels"""
        l = len(rgsw_bits)
        handles = (C.c_void_p * max(1, l))(*[g.handle for g in rgsw_bits])
        _check(lib().sealhip_evaluator_select(self.ctx.handle, k, _ptr(cts), count, l, handles if l else None, _ptr(out)))

    def multiply_monomial(self, ct, k, count, exps, out, n_ct=None, exps_stride=1, minus_one=False):
        """out[i] = X^(e_i) ct[i] - minus_one * ct[i] (sealhip_evaluator_multiply_monomial): e_i =
        exps[i * exps_stride] (uint32, device, reduced mod 2N); ct holds n_ct = count ciphertexts (the default) or 1 shared"""
        _check(lib().sealhip_evaluator_multiply_monomial(self.ctx.handle, k, _ptr(ct), count if n_ct is None else n_ct, count,
                                                         _ptr(exps), exps_stride, 1 if minus_one else 0, _ptr(out)))

    def blind_rotate(self, tv, k, count, exps, rgsw_list, out, n_tv=1):
        """out[i] = X^(exps[i][0]) tv prod_t (1 + (X^(exps[i][t]) - 1) beta_t) in the phase (sealhip_evaluator_blind_rotate):
        tv: n_tv = 1 (shared) or count size-2 ciphertexts; exps: count x (1 + len(rgsw_list)) uint32 (device); rgsw_list[t - 1]
        encrypts the bit beta_t. One streaming launch and one external product per step, the accumulator in out."""
        n = len(rgsw_list)
        handles = (C.c_void_p * max(1, n))(*[g.handle for g in rgsw_list])
        _check(lib().sealhip_evaluator_blind_rotate(self.ctx.handle, k, _ptr(tv), n_tv, count, _ptr(exps), n,
                                                    handles if n else None, _ptr(out)))

    def dot_plain(self, cts, plain, k, count, n_terms, n_sums, out, size=2):
        """Sums against plaintext rows (sealhip_evaluator_dot_plain): out[s] = sum_i ct_i (.) P[s][i],
        everything in NTT form. cts: count x n_terms x size x k x N (the layout expand writes); plain: n_sums x n_terms x k x
        N; out: n_sums x count x size x k x N."""
        _check(lib().sealhip_evaluator_dot_plain(self.ctx.handle, k, _ptr(cts), n_terms, size, count, _ptr(plain), n_sums,
                                                 _ptr(out)))

    def apply_galois_dot_plain(self, ct, k, count, elts, keys, plains, n_sums, out,
                               _entry="sealhip_evaluator_apply_galois_dot_plain"):
        """Plaintext-weighted sums of rotations (sealhip_evaluator_apply_galois_dot_plain):
        out[s] = sum_i plains[s][i] * sigma_{elts[i]}(ct) with one decomposition of c_1 and one mod-down per sum. keys[i] is
        the KSwitchKeys of elts[i] and may be None for element 1. plains: n_sums x len(elts) x n_key x N words in key-level
        NTT form; out: n_sums x count x 2 x k x N, sum-major; ct is not modified."""
        elts = [int(g) for g in elts]
        ea = (_u32 * max(1, len(elts)))(*elts)
        ka = (_vp * max(1, len(elts)))(*[key.handle if key is not None else None for key in keys])
        _check(getattr(lib(), _entry)(self.ctx.handle, k, _ptr(ct), count, ea, ka, len(elts), _ptr(plains), n_sums, _ptr(out)))

    def rotate_vector_dot_plain(self, ct, k, count, steps, galois_keys, plains, n_sums, out,
                                _entry="sealhip_evaluator_rotate_vector_dot_plain"):
        """The same by rotation steps (sealhip_evaluator_rotate_vector_dot_plain): step 0 is the identity and needs no key; a
        step without its key in galois_keys (dict galois_elt -> KSwitchKeys) raises ValueError."""
        steps = [int(st) for st in steps]
        sa = (_i32 * max(1, len(steps)))(*steps)
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(getattr(lib(), _entry)(self.ctx.handle, k, _ptr(ct), count, sa, len(steps), ea, ka, n_keys, _ptr(plains),
                                      n_sums, _ptr(out)))

    def apply_galois_bsgs_plain(self, ct, k, count, baby_elts, baby_keys, giant_elts, giant_keys, plains, out,
                                _entry="sealhip_evaluator_apply_galois_bsgs_plain"):
        """Baby-step/giant-step matrix-vector product (sealhip_evaluator_apply_galois_bsgs_plain):
        out = sum_j sigma_{giant_elts[j]}( sum_i plains[j][i] * sigma_{baby_elts[i]}(ct) ), the giant steps accumulated in the
        extended basis and ONE full mod-down. A key may be None for element 1 on either axis. plains: len(giant_elts) x
        len(baby_elts) x n_key x N words in key-level NTT form; out: count x 2 x k x N; ct is not modified."""
        baby_elts, giant_elts = [int(g) for g in baby_elts], [int(g) for g in giant_elts]
        ba = (_u32 * max(1, len(baby_elts)))(*baby_elts)
        bk = (_vp * max(1, len(baby_elts)))(*[key.handle if key is not None else None for key in baby_keys])
        ga = (_u32 * max(1, len(giant_elts)))(*giant_elts)
        gk = (_vp * max(1, len(giant_elts)))(*[key.handle if key is not None else None for key in giant_keys])
        _check(getattr(lib(), _entry)(self.ctx.handle, k, _ptr(ct), count, ba, bk, len(baby_elts), ga, gk, len(giant_elts),
                                      _ptr(plains), _ptr(out)))

    def rotate_vector_bsgs_plain(self, ct, k, count, baby_steps, giant_steps, galois_keys, plains, out,
                                 _entry="sealhip_evaluator_rotate_vector_bsgs_plain"):
        """The same by rotation steps (sealhip_evaluator_rotate_vector_bsgs_plain): step 0 is the identity and needs no key; a
        step of either axis without its key in galois_keys (dict galois_elt -> KSwitchKeys) raises ValueError."""
        baby_steps, giant_steps = [int(st) for st in baby_steps], [int(st) for st in giant_steps]
        bs = (_i32 * max(1, len(baby_steps)))(*baby_steps)
        gs = (_i32 * max(1, len(giant_steps)))(*giant_steps)
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(getattr(lib(), _entry)(self.ctx.handle, k, _ptr(ct), count, bs, len(baby_steps), gs, len(giant_steps), ea, ka,
                                      n_keys, _ptr(plains), _ptr(out)))

    def dot_product_max_terms(self, k):
        """Terms one dot_product call admits at level k (sealhip_evaluator_dot_product_max_terms): for BFV as many as keep the
        single floor's base conversion exact, for CKKS 2^32 - 1"""
        n = C.c_uint64(0)
        _check(lib().sealhip_evaluator_dot_product_max_terms(self.ctx.handle, k, C.byref(n)))
        return int(n.value)

    def dot_product(self, a_terms, b_terms, k, count, out, relin_keys=None, _entry="sealhip_evaluator_dot_product"):
        """Ciphertext inner product (sealhip_evaluator_dot_product): out = sum_i a_terms[i] * b_terms[i]
        over device batches count x 2 x k x N of size-2 ciphertexts, the tensor products summed in NTT form, one floor (BFV
        STRICT) and, with relin_keys (a list of KSwitchKeys, index 0 is read), one relinearization. out: count x 3 x k x N
        without keys, count x 2 x k x N with them. The operands are not modified; buffers may repeat."""
        if len(a_terms) != len(b_terms):
            raise ValueError("a_terms and b_terms differ in length")
        pa = (_vp * max(1, len(a_terms)))(*[_ptr(c) for c in a_terms])
        pb = (_vp * max(1, len(b_terms)))(*[_ptr(c) for c in b_terms])
        keys, n_relin = _relin_array(relin_keys)
        _check(getattr(lib(), _entry)(self.ctx.handle, k, pa, pb, len(a_terms), count, keys,
                                      n_relin, _ptr(out)))

    def linear_combination(self, terms, weights, k, count, out, size=2, n_sums=1, constant=None):
        """Linear combinations with scalar weights (sealhip_evaluator_linear_combination):
        out[s] = sum_i weights[s][i] * terms[i] (+ constant[s] on polynomial 0) over device batches count x size x k x N.
        weights: device buffer n_sums x len(terms) x k of canonical residues; constant: device buffer n_sums x k or None;
        out: n_sums x count x size x k x N. The operands are not modified; buffers may repeat."""
        pt = (_vp * max(1, len(terms)))(*[_ptr(c) for c in terms])
        _check(lib().sealhip_evaluator_linear_combination(self.ctx.handle, k, pt, len(terms), size, count, _ptr(weights),
                                                          _ptr(constant) if constant is not None else None, n_sums, _ptr(out)))

    def linear_combination_levels(self, terms, term_levels, term_sizes, weights, k, count, out, size=2, n_sums=1, constant=None):
        """linear_combination over CKKS terms that keep their own level and size (sealhip_evaluator_linear_combination_levels,
        DESIGN.md section 21): terms[i] is a device batch count x term_sizes[i] x term_levels[i] x N with term_levels[i] >= k
        and term_sizes[i] <= size, read in place at its first k rows; a term of fewer polynomials contributes nothing to the
        others. weights, constant and out are laid out at level k as for linear_combination. One term with weight 1 is
        mod_switch_to level k in one pass."""
        if not len(terms) == len(term_levels) == len(term_sizes):
            raise ValueError("terms, term_levels and term_sizes differ in length")
        n = max(1, len(terms))
        pt = (_vp * n)(*[_ptr(c) for c in terms])
        lv, sz = (_u32 * n)(*[int(v) for v in term_levels]), (_u32 * n)(*[int(v) for v in term_sizes])
        _check(lib().sealhip_evaluator_linear_combination_levels(self.ctx.handle, k, pt, lv, sz, len(terms), size, count,
                                                                 _ptr(weights), _ptr(constant) if constant is not None else None,
                                                                 n_sums, _ptr(out)))

    def polynomial_plan_ckks(self, k, scale, coeffs, basis=0, n_baby=0, scale_out=0.0, tables=True):
        """The plan of evaluate_polynomial_ckks (sealhip_evaluator_polynomial_plan_ckks); works on a
        host-only context. Returns a dict: d, m, g, inner_level, out_level, n_products, out_scale, temp_bytes_per_item and,
        with tables, the inner sums' weights [g][m - 1][inner_level] and constants [g][inner_level] as uint64 arrays (rows of
        sums that are not formed are zero)."""
        coeffs = [float(c) for c in coeffs]
        if not coeffs:
            raise ValueError("coeffs must not be empty")
        ca = (C.c_double * len(coeffs))(*coeffs)
        plan = PolyPlan()
        fn = lib().sealhip_evaluator_polynomial_plan_ckks
        _check(fn(self.ctx.handle, k, scale, ca, len(coeffs) - 1, basis, n_baby, scale_out, C.addressof(plan), None, None))
        out = {name: getattr(plan, name) for name, _ in PolyPlan._fields_}
        if tables:
            w = np.zeros((plan.g, plan.m - 1, plan.inner_level), dtype=np.uint64)
            kc = np.zeros((plan.g, plan.inner_level), dtype=np.uint64)
            _check(fn(self.ctx.handle, k, scale, ca, len(coeffs) - 1, basis, n_baby, scale_out, C.addressof(plan),
                      w.ctypes.data_as(C.POINTER(_u64)), kc.ctypes.data_as(C.POINTER(_u64))))
            out["weights"], out["constants"] = w, kc
        return out

    def evaluate_polynomial_ckks(self, ct, coeffs, k, count, scale, out, relin_keys=None, basis=0, n_baby=0, scale_out=0.0):
        """p(ct) on CKKS ciphertexts with planned levels and scales (sealhip_evaluator_evaluate_polynomial_ckks, DESIGN.md
        section 21): ct a device batch count x 2 x k x N at `scale`, coeffs host doubles (lowest degree first) in the monomial
        (basis 0) or the Chebyshev basis (1, messages in [-1, 1]); out: count x 2 x out_level x N (polynomial_plan_ckks says
        which level). relin_keys (a list of KSwitchKeys, index 0 is read) may be None for degree one. Returns (out_level,
        out_scale); out_scale is scale_out, or the input scale when that is 0. The words are those of
        tests/poly_eval_ckks_ref.py."""
        coeffs = [float(c) for c in coeffs]
        if not coeffs:
            raise ValueError("coeffs must not be empty")
        ca = (C.c_double * len(coeffs))(*coeffs)
        keys, n_relin = _relin_array(relin_keys)
        level, result_scale = _u32(0), C.c_double(0.0)
        _check(lib().sealhip_evaluator_evaluate_polynomial_ckks(self.ctx.handle, k, _ptr(ct), count, scale, ca, len(coeffs) - 1,
                                                                basis, n_baby, scale_out, keys,
                                                                n_relin, _ptr(out),
                                                                C.byref(level), C.byref(result_scale)))
        return level.value, result_scale.value

    def evaluate_polynomial(self, ct, coeffs, k, count, out, relin_keys=None, n_baby=0):
        """p(ct) = sum_e coeffs[e] ct^e by Paterson-Stockmeyer (sealhip_evaluator_evaluate_polynomial):
        BFV STRICT, ct and out device batches count x 2 x k x N, coeffs host integers below t (lowest degree first), n_baby
        the number of baby steps (0: ceil(sqrt(d + 1))). relin_keys (a list of KSwitchKeys, index 0 is read) may be None for a
        polynomial of degree one. The words are those of tests/poly_eval_ref.py."""
        coeffs = [int(c) for c in coeffs]
        if not coeffs:
            raise ValueError("coeffs must not be empty")
        ca = (C.c_uint64 * len(coeffs))(*coeffs)
        keys, n_relin = _relin_array(relin_keys)
        _check(lib().sealhip_evaluator_evaluate_polynomial(self.ctx.handle, k, _ptr(ct), count, ca, len(coeffs) - 1, n_baby, keys,
                                                           n_relin, _ptr(out)))

    # ---- the key switch's mod-down merged with rescale_to_next: CKKS, operands at level k >= 2, every
    # out at level k - 1; the words are those of tests/ks_rescale_ref.py, the error that of the unmerged method + rescale_to_next
    def relinearize_rescale(self, ct, k, count, relin_keys, out, item_stride=0):
        """relinearize + rescale_to_next in one call (sealhip_evaluator_relinearize_rescale): ct holds count size-3 ciphertexts
        item_stride words apart (0 = back to back) and is not modified; out: count x 2 x (k-1) x N."""
        keys = (_vp * max(1, len(relin_keys)))(*[rk.handle for rk in relin_keys])
        _check(lib().sealhip_evaluator_relinearize_rescale(self.ctx.handle, k, _ptr(ct), 3, item_stride or 3 * k * self.ctx.n,
                                                           count, keys, len(relin_keys), _ptr(out)))

    def dot_product_rescale(self, a_terms, b_terms, k, count, out, relin_keys):
        """dot_product with keys + rescale_to_next in one call (sealhip_evaluator_dot_product_rescale); with one term
        multiply + relinearize + rescale_to_next. out: count x 2 x (k-1) x N."""
        self.dot_product(a_terms, b_terms, k, count, out, relin_keys, _entry="sealhip_evaluator_dot_product_rescale")

    def apply_galois_dot_plain_rescale(self, ct, k, count, elts, keys, plains, n_sums, out):
        """apply_galois_dot_plain + rescale_to_next in one call; out: n_sums x count x 2 x (k-1) x N."""
        self.apply_galois_dot_plain(ct, k, count, elts, keys, plains, n_sums, out,
                                    _entry="sealhip_evaluator_apply_galois_dot_plain_rescale")

    def rotate_vector_dot_plain_rescale(self, ct, k, count, steps, galois_keys, plains, n_sums, out):
        """rotate_vector_dot_plain + rescale_to_next in one call; out: n_sums x count x 2 x (k-1) x N."""
        self.rotate_vector_dot_plain(ct, k, count, steps, galois_keys, plains, n_sums, out,
                                     _entry="sealhip_evaluator_rotate_vector_dot_plain_rescale")

    def apply_galois_bsgs_plain_rescale(self, ct, k, count, baby_elts, baby_keys, giant_elts, giant_keys, plains, out):
        """apply_galois_bsgs_plain + rescale_to_next in one call (the final finish is merged); out: count x 2 x (k-1) x N."""
        self.apply_galois_bsgs_plain(ct, k, count, baby_elts, baby_keys, giant_elts, giant_keys, plains, out,
                                     _entry="sealhip_evaluator_apply_galois_bsgs_plain_rescale")

    def rotate_vector_bsgs_plain_rescale(self, ct, k, count, baby_steps, giant_steps, galois_keys, plains, out):
        """rotate_vector_bsgs_plain + rescale_to_next in one call; out: count x 2 x (k-1) x N."""
        self.rotate_vector_bsgs_plain(ct, k, count, baby_steps, giant_steps, galois_keys, plains, out,
                                      _entry="sealhip_evaluator_rotate_vector_bsgs_plain_rescale")

    # ---- homomorphic DFT: CoeffToSlot / SlotToCoeff
    def dft_plan(self, direction, k, stages, n_baby=None):
        """The plan of a homomorphic DFT (sealhip_evaluator_dft_plan); works on a host-only context. direction:
        DFT_COEFFS_TO_SLOTS or DFT_SLOTS_TO_COEFFS; stages: layer counts in application order, summing to log2(N/2); n_baby:
        per stage or None. Returns a dict: in_level, out_level, needs_conjugation, table_words, temp_bytes_per_item, key_steps
        (the sorted distinct non-zero rotation steps: the Galois keys to make) and stages, a list of dicts s0, r, h0, level,
        n_baby, n_giant, folded, scale, baby_steps, giant_steps."""
        args = _dft_args(direction, k, stages, n_baby)
        plan, key_steps = _plan_with_key_steps(lib().sealhip_evaluator_dft_plan, DftPlan, self.ctx.handle, *args)
        out = _dft_plan_dict(plan)
        out["key_steps"] = key_steps
        for t, st in enumerate(out["stages"]):
            bs, gs = (_i32 * st["n_baby"])(), (_i32 * st["n_giant"])()
            _check(lib().sealhip_dft_stage_steps(self.ctx.handle, *args, t, bs, gs))
            st["baby_steps"], st["giant_steps"] = [int(v) for v in bs], [int(v) for v in gs]
        return out

    def dft_stage_values(self, direction, k, stages, stage, n_baby=None, gain=1.0, host=False):
        """One stage's pre-rotated diagonals as a complex array [n_giant][n_baby][N/2] (sealhip_dft_stage_values: the
        generator kernel, downloaded; host=True: sealhip_dft_stage_values_host, also on a host-only context)."""
        args = _dft_args(direction, k, stages, n_baby)
        plan = DftPlan()
        _check(lib().sealhip_evaluator_dft_plan(self.ctx.handle, *args, C.addressof(plan), None, 0))
        st = plan.stages[stage]
        out = np.zeros((st.n_giant, st.n_baby, self.ctx.n // 2), dtype=np.complex128)
        if host:
            _check(lib().sealhip_dft_stage_values_host(self.ctx.handle, *args, gain, stage, out.ctypes.data))
            return out
        dev = self.ctx.alloc(out.size * 2)
        _check(lib().sealhip_dft_stage_values(self.ctx.handle, *args, gain, stage, dev.ptr))
        return dev.download(out.size * 2).view(np.complex128).reshape(out.shape)

    # ---- matrix-vector products from a caller's matrix
    def linear_transform_plan(self, d, mask=None, n1=0):
        """The plan of a d x d matrix-vector product (sealhip_linear_transform_plan); works on a host-only context. mask: d
        flags, the diagonals in use, or None for all; n1: the baby stride, 0 for the default. Returns a dict: d,
        n_diagonals, n1, n_baby, n_giant, table_words, temp_bytes_per_item, baby_steps, giant_steps and key_steps (the
        sorted distinct non-zero rotation steps: the Galois keys to make)."""
        m = _mask_bytes(mask, d)
        plan = LintransPlan()
        fn = lib().sealhip_linear_transform_plan
        _check(fn(self.ctx.handle, d, _np_ptr(m), n1, C.addressof(plan), None, None, None, 0))
        cap = max(1, plan.n_baby, plan.n_giant, plan.n_key_steps)
        bs, gs, ks = (_i32 * cap)(), (_i32 * cap)(), (_u32 * cap)()
        _check(fn(self.ctx.handle, d, _np_ptr(m), n1, C.addressof(plan), bs, gs, ks, cap))
        out = _lintrans_plan_dict(plan)
        out["baby_steps"], out["giant_steps"] = [int(v) for v in bs[:plan.n_baby]], [int(v) for v in gs[:plan.n_giant]]
        out["key_steps"] = [int(v) for v in ks[:plan.n_key_steps]]
        return out

    def linear_transform_diagonals(self, matrix, d):
        """The diagonals of a device matrix that hold a non-zero entry, as d flags (sealhip_linear_transform_diagonals: the
        occupancy kernel); a non-finite entry raises ValueError. matrix: d x d complex doubles in device memory."""
        out = np.zeros(d, dtype=np.uint8)
        _check(lib().sealhip_linear_transform_diagonals(self.ctx.handle, _ptr(matrix), d, out.ctypes.data))
        return out

    def linear_transform_values(self, matrix, d, mask=None, n1=0, gain=1.0, host=False):
        """The pre-rotated diagonals as a complex array [n_giant][n_baby][N/2] (sealhip_linear_transform_values: the gather
        kernel over a device matrix, downloaded; host=True: matrix is a numpy array and sealhip_linear_transform_values_host
        does the same on the host, also on a host-only context)."""
        plan = self.linear_transform_plan(d, mask, n1)
        m = _mask_bytes(mask, d)
        out = np.zeros((plan["n_giant"], plan["n_baby"], self.ctx.n // 2), dtype=np.complex128)
        if host:
            mat = np.ascontiguousarray(matrix, dtype=np.complex128)
            if mat.size != d * d:
                raise ValueError("matrix is not d x d")
            _check(lib().sealhip_linear_transform_values_host(self.ctx.handle, mat.ctypes.data, d, _np_ptr(m), n1, gain,
                                                              out.ctypes.data))
            return out
        dev = self.ctx.alloc(out.size * 2)
        _check(lib().sealhip_linear_transform_values(self.ctx.handle, _ptr(matrix), d, _np_ptr(m), n1, gain, dev.ptr))
        return dev.download(out.size * 2).view(np.complex128).reshape(out.shape)

    def linear_transform(self, tables, ct, k, count, galois_keys, out, rescale=False):
        """out = the tables' matrix applied to the slots of ct (sealhip_evaluator_linear_transform): ct a device batch
        count x 2 x k x N; out: count x 2 x k x N, or count x 2 x (k-1) x N with rescale. galois_keys: dict galois_elt ->
        KSwitchKeys with the plan's key_steps; a missing one raises ValueError. The scale is multiplied by tables.scale
        (and divided by q_(k-1) with rescale)."""
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(lib().sealhip_evaluator_linear_transform(self.ctx.handle, tables.handle, k, _ptr(ct), count, ea, ka, n_keys,
                                                        1 if rescale else 0, _ptr(out)))

    def coeffs_to_slots(self, tables, ct, count, galois_keys, out_re, out_im):
        """CoeffToSlot in one call (sealhip_evaluator_coeffs_to_slots): ct a device batch count x 2 x k x N at the tables'
        level; out_re, out_im: count x 2 x tables.out_level x N, slot j of them m_(bitrev j) and m_(bitrev j + N/2) over the
        scale, which is unchanged. galois_keys: dict galois_elt -> KSwitchKeys with the plan's key_steps and element 2N - 1;
        a missing one raises ValueError."""
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(lib().sealhip_evaluator_coeffs_to_slots(self.ctx.handle, tables.handle, _ptr(ct), count, ea, ka, n_keys,
                                                       _ptr(out_re), _ptr(out_im)))

    def slots_to_coeffs(self, tables, ct_re, ct_im, count, galois_keys, out):
        """SlotToCoeff in one call (sealhip_evaluator_slots_to_coeffs): ct_re, ct_im device batches count x 2 x k x N in
        coeffs_to_slots' bit-reversed slot order; out: count x 2 x tables.out_level x N; the scale is unchanged."""
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(lib().sealhip_evaluator_slots_to_coeffs(self.ctx.handle, tables.handle, _ptr(ct_re), _ptr(ct_im), count, ea, ka,
                                                       n_keys, _ptr(out)))

    # ---- towards CKKS bootstrapping: ModRaise and the double-angle step
    def mod_raise(self, ct, k_in, count, k_out, out):
        """ModRaise (sealhip_evaluator_mod_raise): ct a device batch count x 2 x k_in x N in NTT form, of which only the q_0
        rows are read; out: count x 2 x k_out x N, the centred coefficients modulo q_0 re-read modulo q_0 .. q_(k_out-1). The
        result decrypts to m + q_0 I. Both buffers must be 16-byte aligned."""
        _check(lib().sealhip_evaluator_mod_raise(self.ctx.handle, k_in, _ptr(ct), count, k_out, _ptr(out)))

    def double_angle(self, ct, k, count, scale, relin_keys, out):
        """out = 2 ct^2 - 1 from level k to k - 1 in one call (sealhip_evaluator_double_angle): ct a device batch
        count x 2 x k x N at `scale`, 16-byte aligned, out: count x 2 x (k-1) x N. Returns the result's scale, scale * scale / q_(k-1). The words
        are those of dot_product without keys, linear_combination_levels and relinearize_rescale issued one by one."""
        keys, n_relin = _relin_array(relin_keys)
        out_scale = C.c_double(0.0)
        _check(lib().sealhip_evaluator_double_angle(self.ctx.handle, k, _ptr(ct), count, scale, keys,
                                                    n_relin, _ptr(out),
                                                    C.byref(out_scale)))
        return out_scale.value

    def evalmod_plan(self, k, scale, K, r, degree, n_baby=0, scale_out=0.0):
        """The plan of eval_mod (sealhip_evaluator_evalmod_plan); works on a host-only context. Returns a dict: K, r, degree,
        n_baby, poly_level, out_level, n_products, poly_scale_out (t_0), scales [s_0 .. s_r], out_scale (s_r),
        temp_bytes_per_item and coeffs, the Chebyshev coefficients (sealhip_evalmod_coeffs)."""
        plan = EvalModPlan()
        _check(lib().sealhip_evaluator_evalmod_plan(self.ctx.handle, k, scale, K, r, degree, n_baby, scale_out,
                                                    C.addressof(plan)))
        out = _evalmod_plan_dict(plan)
        out["coeffs"] = evalmod_coeffs(K, r, degree)
        return out

    def eval_mod(self, ct, k, count, scale, K, r, degree, relin_keys, out, n_baby=0, scale_out=0.0):
        """EvalMod in one call (sealhip_evaluator_eval_mod): ct a device batch count x 2 x k x N whose slots hold
        x = c / (q_0 K) in [-1, 1] at `scale`; out: count x 2 x out_level x N, slots sin(2 pi K x) (evalmod_plan says which
        level). Returns (out_level, out_scale)."""
        keys, n_relin = _relin_array(relin_keys)
        level, result_scale = _u32(0), C.c_double(0.0)
        _check(lib().sealhip_evaluator_eval_mod(self.ctx.handle, k, _ptr(ct), count, scale, K, r, degree, n_baby, scale_out, keys,
                                                n_relin, _ptr(out), C.byref(level),
                                                C.byref(result_scale)))
        return level.value, result_scale.value

    def bootstrap_plan(self, k_top, c2s_stages, s2c_stages, K, r, degree, n_baby=0, c2s_n_baby=None, s2c_n_baby=None):
        """The plan of a bootstrap (sealhip_evaluator_bootstrap_plan); works on a host-only context. Returns a dict: k_top,
        c2s_out_level, evalmod_out_level, out_level, needs_conjugation, raise_scale S = q_0 K, s2c_gain, table_words,
        temp_bytes_per_item, key_steps (the sorted distinct rotation steps of both transforms: the Galois keys to make, next
        to element 2N - 1) and evalmod, the dict of evalmod_plan."""
        args = _bootstrap_args(k_top, c2s_stages, c2s_n_baby, s2c_stages, s2c_n_baby, K, r, degree, n_baby)
        plan, key_steps = _plan_with_key_steps(lib().sealhip_evaluator_bootstrap_plan, BootstrapPlan, self.ctx.handle, *args)
        out = _bootstrap_plan_dict(plan)
        out["key_steps"] = key_steps
        return out

    def bootstrap(self, tables, ct, k_in, count, galois_keys, relin_keys, out):
        """Bootstrap in one call (sealhip_evaluator_bootstrap): ct a device batch count x 2 x k_in x N (only the q_0 rows are
        read); out: count x 2 x tables.plan["out_level"] x N at the input's scale. galois_keys: dict galois_elt ->
        KSwitchKeys with the plan's key_steps and element 2N - 1; relin_keys: a list of KSwitchKeys (index 0 is read)."""
        ea, ka, n_keys = _galois_arrays(galois_keys)
        keys, n_relin = _relin_array(relin_keys)
        _check(lib().sealhip_evaluator_bootstrap(self.ctx.handle, tables.handle, k_in, _ptr(ct), count, ea, ka, n_keys, keys,
                                                 n_relin, _ptr(out)))

    # ---- sparse-secret encapsulation
    def switch_secret(self, ct, k, count, key, out):
        """Re-encryption under another secret (sealhip_evaluator_switch_secret): out = (c_0, 0) + switch_key(c_1) of the
        device batch ct count x 2 x k x N; key: a KSwitchKeys of Context.generate_switching_keys."""
        _check(lib().sealhip_evaluator_switch_secret(self.ctx.handle, k, _ptr(ct), count, key.handle if key is not None else None,
                                                     _ptr(out)))

    def bootstrap_encapsulated(self, tables, ct, k_in, count, galois_keys, relin_keys, to_sparse, to_dense, out):
        """bootstrap with ModRaise alone under a sparse secret (sealhip_evaluator_bootstrap_encapsulated): to_sparse the
        dense -> sparse switching key made with level 1, to_dense the sparse -> dense one at the full level; everything else
        as bootstrap, under the dense secret."""
        ea, ka, n_keys = _galois_arrays(galois_keys)
        keys, n_relin = _relin_array(relin_keys)
        _check(lib().sealhip_evaluator_bootstrap_encapsulated(
            self.ctx.handle, tables.handle, k_in, _ptr(ct), count, ea, ka, n_keys, keys, n_relin,
            to_sparse.handle if to_sparse is not None else None, to_dense.handle if to_dense is not None else None, _ptr(out)))

    # ---- batches of separately allocated HOST ciphertexts (lists of numpy arrays: what a vector<Ciphertext> is)
    @staticmethod
    def _host_ptrs(arrays):
        for a in arrays:
            assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
        return (C.c_void_p * max(1, len(arrays)))(*[a.ctypes.data for a in arrays])

    def host_register(self, array):
        """sealhip_host_register: pins the array's memory in place; *_host entries then copy it without staging"""
        _check(lib().sealhip_host_register(self.ctx.handle, array.ctypes.data, array.nbytes))

    def host_unregister(self, array):
        _check(lib().sealhip_host_unregister(self.ctx.handle, array.ctypes.data))

    def multiply_host(self, a, size_a, b, size_b, k, out, relin_keys=None):
        """Evaluator::multiply (+ relinearize when relin_keys is given) over lists of host ciphertexts; out[i] is written"""
        keys = (C.c_void_p * max(1, len(relin_keys or [])))(*[rk.handle for rk in (relin_keys or [])])
        _check(lib().sealhip_evaluator_multiply_host(self.ctx.handle, k, self._host_ptrs(a), size_a, self._host_ptrs(b), size_b,
                                                     len(a), self._host_ptrs(out), keys if relin_keys else None,
                                                     len(relin_keys or [])))

    def relinearize_host(self, cts, size, k, relin_keys):
        keys = (C.c_void_p * max(1, len(relin_keys)))(*[rk.handle for rk in relin_keys])
        _check(lib().sealhip_evaluator_relinearize_host(self.ctx.handle, k, self._host_ptrs(cts), size, len(cts), keys,
                                                        len(relin_keys)))

    def rotate_vector_host(self, cts, k, steps, galois_keys):
        ea, ka, n_keys = _galois_arrays(galois_keys)
        _check(lib().sealhip_evaluator_rotate_vector_host(self.ctx.handle, k, self._host_ptrs(cts), len(cts), steps, ea, ka,
                                                          n_keys))

    def mod_switch_to_next_host(self, cts, size, k, out, rescale=False):
        fn = lib().sealhip_evaluator_rescale_to_next_host if rescale else lib().sealhip_evaluator_mod_switch_to_next_host
        _check(fn(self.ctx.handle, k, self._host_ptrs(cts), size, len(cts), self._host_ptrs(out)))

    # ---- the rest of the Evaluator surface on device-resident batches
    def negate(self, ct, size, k, count, out):
        """Evaluator::negate (evaluator.cpp:65-88)"""
        _check(lib().sealhip_evaluator_negate(self.ctx.handle, k, _ptr(ct), size, count, _ptr(out)))

    def add(self, a, size_a, b, size_b, k, count, out):
        """Evaluator::add (evaluator.cpp:90-151)"""
        _check(lib().sealhip_evaluator_add(self.ctx.handle, k, _ptr(a), size_a, _ptr(b), size_b, count, _ptr(out)))

    def sub(self, a, size_a, b, size_b, k, count, out):
        """Evaluator::sub (evaluator.cpp:174-233)"""
        _check(lib().sealhip_evaluator_sub(self.ctx.handle, k, _ptr(a), size_a, _ptr(b), size_b, count, _ptr(out)))

    def multiply_plain_inplace(self, ct, size, k, count, plain, plain_stride=0, ntt_form=None):
        """Evaluator::multiply_plain_inplace (evaluator.cpp:1438-1473): NTT form -> multiply_plain_ntt (plain = k x N in
        NTT form), coefficient form (BFV) -> multiply_plain_normal (plain = N coefficients < t)."""
        if ntt_form is None:
            ntt_form = self.ctx.scheme == SCHEME_CKKS
        fn = lib().sealhip_evaluator_multiply_plain_ntt if ntt_form else lib().sealhip_evaluator_multiply_plain
        _check(fn(self.ctx.handle, k, _ptr(ct), size, count, _ptr(plain), plain_stride))

    def transform_plain_to_ntt(self, plain, coeff_count, k, count, plain_ntt, plain_stride=0):
        """Evaluator::transform_to_ntt(Plaintext, parms_id) (evaluator.cpp:1648-1744), BFV: `count` plaintexts of coeff_count
        coefficients < t (plain_stride words apart, 0 = coeff_count) -> plain_ntt[count][k][N] in NTT form at level k"""
        _check(lib().sealhip_evaluator_transform_plain_to_ntt(self.ctx.handle, k, _ptr(plain), coeff_count, plain_stride, count,
                                                               _ptr(plain_ntt)))

    def mod_switch_plain_to(self, plain, k_from, count, k_to, out):
        """Evaluator::mod_switch_to(Plaintext, parms_id) (evaluator.cpp:1062-1088): NTT-form plain[count][k_from][N] ->
        out[count][k_to][N]"""
        _check(lib().sealhip_evaluator_mod_switch_plain_to(self.ctx.handle, k_from, _ptr(plain), count, k_to, _ptr(out)))

    def add_plain_inplace(self, ct, size, k, count, plain, plain_stride=None, subtract=False):
        """Evaluator::add_plain_inplace / sub_plain_inplace (evaluator.cpp:1290-1435): BFV plain = N coefficients < t,
        CKKS plain = k x N in NTT form"""
        if plain_stride is None:
            plain_stride = self.ctx.n if self.ctx.scheme == SCHEME_BFV else k * self.ctx.n
        _check(lib().sealhip_evaluator_add_plain(self.ctx.handle, k, _ptr(ct), size, count, _ptr(plain), plain_stride,
                                                 1 if subtract else 0))

    def sub_plain_inplace(self, ct, size, k, count, plain, plain_stride=None):
        self.add_plain_inplace(ct, size, k, count, plain, plain_stride, subtract=True)

    def resize(self, src, src_size, dst_size, k, count, dst=None):
        """Ciphertext::resize (ciphertext.cpp:84-124) over a batch; returns the destination buffer"""
        if dst is None:
            dst = self.ctx.alloc(count * dst_size * k * self.ctx.n)
        _check(lib().sealhip_ciphertext_resize(self.ctx.handle, k, _ptr(src), src_size, _ptr(dst), dst_size, count))
        return dst

    def add_many(self, cts, size, k, count, out):
        """Evaluator::add_many (evaluator.cpp:153-172): out = cts[0] + cts[1] + ... (left to right)"""
        if not cts:
            raise ValueError("encrypteds cannot be empty")
        self.add(cts[0], size, cts[1], size, k, count, out) if len(cts) > 1 else self.resize(cts[0], size, size, k, count, out)
        for c in cts[2:]:
            self.add(out, size, c, size, k, count, out)

    def multiply_many(self, cts, k, count, relin_keys):
        """Evaluator::multiply_many (evaluator.cpp:1180-1255), BFV, size-2 operands, behind the C ABI
        (sealhip_evaluator_multiply_many): the reference's queue order, each product relinearized. Returns the device buffer
        of the result ([count][2][k][N])."""
        out = self.ctx.alloc(count * 2 * k * self.ctx.n)
        ptrs = (C.c_void_p * max(1, len(cts)))(*[_ptr(c) for c in cts])
        keys = (C.c_void_p * max(1, len(relin_keys)))(*[rk.handle for rk in relin_keys])
        _check(lib().sealhip_evaluator_multiply_many(self.ctx.handle, k, ptrs, len(cts), count, keys, len(relin_keys), _ptr(out)))
        return out

    def exponentiate(self, ct, exponent, k, count, relin_keys):
        """Evaluator::exponentiate_inplace (evaluator.cpp:1257-1288) behind the C ABI (sealhip_evaluator_exponentiate)"""
        out = self.ctx.alloc(count * 2 * k * self.ctx.n)
        keys = (C.c_void_p * max(1, len(relin_keys)))(*[rk.handle for rk in relin_keys])
        _check(lib().sealhip_evaluator_exponentiate(self.ctx.handle, k, _ptr(ct), int(exponent), count, keys, len(relin_keys),
                                                    _ptr(out)))
        return out

    def mod_switch_to(self, ct, size, k, k_target, count):
        """Evaluator::mod_switch_to_inplace (evaluator.cpp:1038-1088): mod_switch_to_next until level k_target"""
        if k_target > k:
            raise ValueError("cannot switch to higher level modulus")
        cur = ct
        while k > k_target:
            nxt = self.ctx.alloc(count * size * (k - 1) * self.ctx.n)
            self.mod_switch_to_next(cur, size, k, count, nxt)
            cur, k = nxt, k - 1
        return cur

    def rescale_to(self, ct, size, k, k_target, count):
        """Evaluator::rescale_to_inplace (evaluator.cpp:1128-1178), CKKS"""
        if k_target > k:
            raise ValueError("cannot switch to higher level modulus")
        cur = ct
        while k > k_target:
            nxt = self.ctx.alloc(count * size * (k - 1) * self.ctx.n)
            self.rescale_to_next(cur, size, k, count, nxt)
            cur, k = nxt, k - 1
        return cur

    def check_not_transparent(self, ct, size, k, count):
        """evaluator.cpp:265-271 (SEAL_THROW_ON_TRANSPARENT_CIPHERTEXT)"""
        if self.ctx.is_transparent(ct, size, k, count).any():
            raise LogicError("result ciphertext is transparent")

    def transform_to_ntt_inplace(self, ct, size, k, count):
        _check(lib().sealhip_evaluator_transform_to_ntt(self.ctx.handle, k, _ptr(ct), size, count))

    def transform_from_ntt_inplace(self, ct, size, k, count):
        _check(lib().sealhip_evaluator_transform_from_ntt(self.ctx.handle, k, _ptr(ct), size, count))


def evalmod_coeffs(K, r, degree):
    """The Chebyshev coefficients of cos((2 pi K x - pi / 2) / 2^r) by interpolation at degree + 1 nodes
    (sealhip_evalmod_coeffs), lowest degree first"""
    out = (C.c_double * (max(0, int(degree)) + 1))()
    _check(lib().sealhip_evalmod_coeffs(K, r, degree, out))
    return [float(v) for v in out]


def _u32_array(values):
    return (_u32 * max(1, len(values)))(*[int(v) for v in values]) if values is not None else None


def _relin_array(relin_keys):
    """(the handles of a list of KSwitchKeys or None, their number): the ABI's relin_keys, n_relin_keys"""
    if relin_keys is None:
        return None, 0
    return (_vp * max(1, len(relin_keys)))(*[rk.handle for rk in relin_keys]), len(relin_keys)


def _galois_arrays(galois_keys):
    """(elements, key handles, their number) of a dict galois_elt -> KSwitchKeys: the ABI's galois_elts, galois_keys, n_keys"""
    elts = list(galois_keys.keys())
    return (_u32 * max(1, len(elts)))(*elts), (_vp * max(1, len(elts)))(*[galois_keys[g].handle for g in elts]), len(elts)


def _plan_with_key_steps(fn, plan_type, *args):
    """The ABI's two calls of a plan entry: the plan, which says how many key steps there are, then the steps"""
    plan = plan_type()
    _check(fn(*args, C.addressof(plan), None, 0))
    steps = (_u32 * max(1, plan.n_key_steps))()
    _check(fn(*args, C.addressof(plan), steps, plan.n_key_steps))
    return plan, [int(v) for v in steps[:plan.n_key_steps]]


def _evalmod_plan_dict(plan):
    out = {name: getattr(plan, name) for name, _ in EvalModPlan._fields_ if name not in ("scales", "reserved")}
    out["scales"] = [float(v) for v in plan.scales[:plan.r + 1]]
    out["out_scale"] = out["scales"][-1]
    return out


class _Tables:
    """A handle of device tables and its end: free() destroys them once and raises when the library refuses (during a graph
    capture), in which case the handle is kept"""
    _destroy = None  # the ABI's destroy entry, by name

    def __init__(self, ctx):
        self.ctx, self.handle = ctx, _vp()

    def free(self):
        if self.handle and lib is not None:
            _check(getattr(lib(), self._destroy)(self.handle))
            self.handle = _vp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _bootstrap_args(k_top, c2s_stages, c2s_n_baby, s2c_stages, s2c_n_baby, K, r, degree, n_baby):
    for stages, nb in ((c2s_stages, c2s_n_baby), (s2c_stages, s2c_n_baby)):
        if nb is not None and len(nb) != len(stages):
            raise ValueError("n_baby and stages differ in length")
    return (k_top, _u32_array(c2s_stages), len(c2s_stages), _u32_array(c2s_n_baby), _u32_array(s2c_stages), len(s2c_stages),
            _u32_array(s2c_n_baby), K, r, degree, n_baby)


def _bootstrap_plan_dict(plan):
    out = {name: getattr(plan, name) for name, _ in BootstrapPlan._fields_ if name not in ("evalmod", "n_key_steps")}
    out["evalmod"] = _evalmod_plan_dict(plan.evalmod)
    return out


class BootstrapTables(_Tables):
    """sealhip_bootstrap_tables: both transforms' tables, the EvalMod coefficients and the intermediates' pool blocks of
    one bootstrap shape"""
    _destroy = "sealhip_bootstrap_tables_destroy"

    def __init__(self, ctx, k_top, c2s_stages, s2c_stages, K, r, degree, n_baby=0, c2s_n_baby=None, s2c_n_baby=None):
        super().__init__(ctx)
        args = _bootstrap_args(k_top, c2s_stages, c2s_n_baby, s2c_stages, s2c_n_baby, K, r, degree, n_baby)
        _check(lib().sealhip_bootstrap_tables_create(ctx.handle, *args, C.byref(self.handle)))
        plan = BootstrapPlan()
        _check(lib().sealhip_bootstrap_tables_plan(self.handle, C.addressof(plan)))
        self.plan = _bootstrap_plan_dict(plan)


def _dft_args(direction, k, stages, n_baby):
    sa = _u32_array(stages)
    if n_baby is not None and len(n_baby) != len(stages):
        raise ValueError("n_baby and stages differ in length")
    return int(direction), int(k), sa, len(stages), _u32_array(n_baby)


def _dft_plan_dict(plan):
    out = {name: int(getattr(plan, name)) for name in ("direction", "in_level", "out_level", "needs_conjugation", "table_words",
                                                        "temp_bytes_per_item")}
    out["stages"] = []
    for t in range(plan.n_stages):
        st = plan.stages[t]
        d = {name: int(getattr(st, name)) for name in ("s0", "r", "h0", "level", "n_baby", "n_giant", "folded")}
        d["scale"] = float(st.scale)
        out["stages"].append(d)
    return out


class DftTables(_Tables):
    """The device tables of one homomorphic DFT (sealhip_dft_tables_create): every stage's diagonals,
    generated on the device and encoded at the key level. plan: Evaluator.dft_plan's dict without the step lists;
    stage_ptr(t): the device address of stage t's n_giant x n_baby x n_key x N words."""

    _destroy = "sealhip_dft_tables_destroy"

    def __init__(self, ctx, direction, k, stages, n_baby=None, gain=1.0):
        super().__init__(ctx)
        _check(lib().sealhip_dft_tables_create(ctx.handle, *_dft_args(direction, k, stages, n_baby), gain,
                                               C.byref(self.handle)))
        plan = DftPlan()
        _check(lib().sealhip_dft_tables_plan(self.handle, C.addressof(plan)))
        self.plan = _dft_plan_dict(plan)
        self.in_level, self.out_level = self.plan["in_level"], self.plan["out_level"]

    def stage_ptr(self, stage):
        p = _vp()
        _check(lib().sealhip_dft_tables_stage(self.handle, stage, C.byref(p)))
        return p.value


def _mask_bytes(mask, d):
    """the ABI's diag_mask_host: d bytes, or None for every diagonal"""
    if mask is None:
        return None
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    if m.size != d:
        raise ValueError("mask must have d entries")
    return m


def _np_ptr(a):
    return a.ctypes.data if a is not None else None


def _lintrans_plan_dict(plan):
    return {name: int(getattr(plan, name)) for name, _ in LintransPlan._fields_ if name != "n_key_steps"}


class LinearTransform(_Tables):
    """The device tables of one d x d matrix (sealhip_linear_transform_create): the diagonals that
    hold a non-zero entry, found, pre-rotated and encoded at the key level on the device. matrix: d x d complex doubles in
    device memory (a DeviceBuffer, a torch tensor or an address). plan: Evaluator.linear_transform_plan's dict for the
    diagonals found; scale: of the plaintexts; plain_ptr(): the device address of the n_giant x n_baby x n_key x N words."""

    _destroy = "sealhip_linear_transform_destroy"

    def __init__(self, ctx, matrix, d, scale, n1=0, gain=1.0):
        super().__init__(ctx)
        _check(lib().sealhip_linear_transform_create(ctx.handle, _ptr(matrix), d, n1, scale, gain, C.byref(self.handle)))
        plan, sc = LintransPlan(), C.c_double(0.0)
        _check(lib().sealhip_linear_transform_tables_plan(self.handle, C.addressof(plan), C.byref(sc)))
        self.plan, self.scale = _lintrans_plan_dict(plan), sc.value
        bs, gs = (_i32 * max(1, plan.n_baby))(), (_i32 * max(1, plan.n_giant))()
        _check(lib().sealhip_linear_transform_tables_steps(self.handle, bs, gs))
        self.plan["baby_steps"] = [int(v) for v in bs[:plan.n_baby]]
        self.plan["giant_steps"] = [int(v) for v in gs[:plan.n_giant]]
        self.plan["key_steps"] = sorted({s for s in self.plan["baby_steps"] + self.plan["giant_steps"] if s})

    def plain_ptr(self):
        p = _vp()
        _check(lib().sealhip_linear_transform_tables_plain(self.handle, C.byref(p)))
        return p.value


def _naf(value):
    """util/numth.h:22-42"""
    res, sign, value, i = [], value < 0, abs(value), 0
    while value:
        zi = 2 - (value % 4) if value % 2 else 0
        value = (value - zi) // 2
        if zi:
            res.append((-zi if sign else zi) * (1 << i))
        i += 1
    return res

"""ctypes binding of include/bbg.h (libbbg.so).  Host arrays are numpy uint64 in the reference's layout:
scalars / coefficients (n, 4); affine points (n, 8); Jacobian points (n, 12) or (12,)."""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("BBG_LIB_PATH") or os.path.join(CSRC, "libbbg.so")  # BBG_LIB_PATH: A/B builds of the same ABI (tests/tools), never a fallback

# op codes of bbg_ntt (include/bbg.h)
FFT, IFFT, COSET_FFT, COSET_IFFT = 0, 1, 2, 3
FFT_WITH_CONSTANT, COSET_FFT_WITH_CONSTANT, COSET_FFT_WITH_GENERATOR_SHIFT, IFFT_WITH_CONSTANT = 4, 5, 6, 7
# forms of bbg_wire_decode / bbg_wire_encode (include/bbg.h)
WIRE_G1_COMPRESSED, WIRE_G1_COMPRESSED_BYTES, WIRE_G1_BUFFER, WIRE_FR, WIRE_FR_BYTES = 0, 1, 2, 3, 4


class BbgError(RuntimeError):
    pass


def build_library(force=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True)
    return LIB_PATH


_lib = None


def load_library():
    """dlopen libbbg.so and declare prototypes.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BbgError(f"{LIB_PATH} is missing: run __graft_entry__.build() (there is no CPU fallback)")
    # One HIP runtime per process.  The PyTorch wheel bundles its own libamdhip64 (soname libamdhip64.so.7, the
    # same soname libbbg.so needs).  If torch is imported AFTER libbbg pulled in /opt/rocm's copy, torch loads a
    # second runtime by file name and finds "No HIP GPUs".  Importing torch first makes the loader resolve
    # libbbg's NEEDED entry to the copy torch already mapped, so both share devices, streams and allocations.
    if os.environ.get("BBG_NO_TORCH") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = ctypes.CDLL(LIB_PATH)
    vp, sz, u64p, cint = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int
    protos = {
        "bbg_device_count": (cint, []),
        "bbg_init": (cint, [cint, ctypes.POINTER(vp)]),
        "bbg_destroy": (None, [vp]),
        "bbg_last_error": (ctypes.c_char_p, []),
        "bbg_sync": (cint, [vp]),
        "bbg_join": (cint, [vp]),
        "bbg_join_lag": (cint, [vp, cint]),
        "bbg_set_stream": (cint, [vp, vp]),
        "bbg_srs_register": (cint, [vp, vp, sz, sz, ctypes.POINTER(vp)]),
        "bbg_srs_register_device": (cint, [vp, vp, sz, ctypes.POINTER(vp)]),
        "bbg_srs_synth_linear": (cint, [vp, ctypes.c_uint64, ctypes.c_uint64, sz, ctypes.POINTER(vp)]),
        "bbg_srs_synth_hashed": (cint, [vp, ctypes.c_uint64, sz, ctypes.POINTER(vp)]),
        "bbg_srs_synth_powers": (cint, [vp, vp, sz, ctypes.POINTER(vp)]),
        "bbg_srs_load_transcript": (cint, [vp, ctypes.c_char_p, sz, ctypes.POINTER(vp)]),
        "bbg_srs_register_transcript_buffer": (cint, [vp, vp, sz, ctypes.POINTER(vp)]),
        "bbg_srs_write_transcript": (cint, [vp, ctypes.c_char_p, sz, vp]),
        "bbg_transcript_checksum": (cint, [vp, sz, vp]),
        "bbg_srs_num_points": (sz, [vp]),
        "bbg_srs_read": (cint, [vp, sz, sz, vp]),
        "bbg_srs_free": (None, [vp]),
        "bbg_srs_retain": (cint, [vp]),
        "bbg_srs_lagrange": (cint, [vp, vp, ctypes.c_uint, ctypes.POINTER(vp)]),
        "bbg_msm": (cint, [vp, vp, vp, sz, sz, vp]),
        "bbg_msm_device": (cint, [vp, vp, vp, sz, sz, vp]),
        "bbg_msm_batch": (cint, [vp, vp, sz, vp, vp, vp, vp]),
        "bbg_msm_batch_device": (cint, [vp, vp, sz, vp, vp, vp, vp]),
        "bbg_msm_plan": (cint, [vp, vp, sz, ctypes.POINTER(cint), ctypes.POINTER(cint)]),
        "bbg_ntt_plan": (cint, [vp, ctypes.c_uint, ctypes.POINTER(cint), ctypes.POINTER(cint), ctypes.POINTER(cint), ctypes.POINTER(cint)]),
        "bbg_memory_report": (cint, [vp, vp]),
        "bbg_memory_trim": (cint, [vp, cint, ctypes.POINTER(sz)]),
        "bbg_prover_device_bytes": (cint, [vp, ctypes.POINTER(sz)]),
        "bbg_g1_sum": (cint, [vp, vp, sz, vp]),
        "bbg_g1_sum_device": (cint, [vp, vp, sz, vp]),
        "bbg_g1_normalize": (cint, [vp, vp, sz, vp]),
        "bbg_g1_fixed_base_mul": (cint, [vp, vp, vp, sz, vp]),
        "bbg_g1_fixed_base_mul_device": (cint, [vp, vp, vp, sz, vp]),
        "bbg_g1_batch_mul": (cint, [vp, vp, vp, sz, cint, vp]),
        "bbg_g1_batch_mul_device": (cint, [vp, vp, vp, sz, cint, vp]),
        "bbg_srs_scale_powers": (cint, [vp, vp, vp, ctypes.POINTER(vp)]),
        "bbg_g1_msm": (cint, [vp, vp, vp, sz, cint, vp]),
        "bbg_g1_msm_device": (cint, [vp, vp, vp, sz, cint, vp]),
        "bbg_g1_msm_plan": (cint, [sz, cint, ctypes.POINTER(cint), ctypes.POINTER(cint), ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "bbg_g2_mul": (cint, [vp, vp, vp, sz, vp]),
        "bbg_g2_lines_prepare": (cint, [vp, vp, sz, ctypes.POINTER(vp)]),
        "bbg_g2_lines_pairs": (cint, [vp, ctypes.POINTER(sz)]),
        "bbg_g2_lines_read": (cint, [vp, sz, vp]),
        "bbg_g2_lines_free": (None, [vp]),
        "bbg_pairing_product_device": (cint, [vp, vp, vp, sz, vp, vp]),
        "bbg_pairing_product": (cint, [vp, vp, vp, sz, vp, vp]),
        "bbg_pairing_product_wave_device": (cint, [vp, vp, vp, sz, vp, vp]),
        "bbg_pairing_product_wave": (cint, [vp, vp, vp, sz, vp, vp]),
        "bbg_g1_ntt": (cint, [vp, vp, ctypes.c_uint, cint, vp]),
        "bbg_g1_ntt_device": (cint, [vp, vp, ctypes.c_uint, cint, vp]),
        "bbg_open_all_prepare": (cint, [vp, vp, ctypes.c_uint, ctypes.POINTER(vp)]),
        "bbg_open_all_prepare_cells": (cint, [vp, vp, ctypes.c_uint, ctypes.c_uint, ctypes.POINTER(vp)]),
        "bbg_open_all_count": (cint, [vp, ctypes.POINTER(sz)]),
        "bbg_open_all_device": (cint, [vp, vp, vp]),
        "bbg_open_all": (cint, [vp, vp, vp]),
        "bbg_open_all_device_bytes": (cint, [vp, ctypes.POINTER(sz)]),
        "bbg_open_all_batch_reserve": (cint, [vp, sz]),
        "bbg_open_all_batch_device": (cint, [vp, vp, sz, vp]),
        "bbg_open_all_batch": (cint, [vp, vp, sz, vp]),
        "bbg_open_all_free": (None, [vp]),
        "bbg_cells_values_device": (cint, [vp, vp, ctypes.c_uint, ctypes.c_uint, sz, vp]),
        "bbg_cells_values": (cint, [vp, vp, ctypes.c_uint, ctypes.c_uint, sz, vp]),
        "bbg_cells_recover_device": (cint, [vp, vp, sz, vp, ctypes.c_uint, ctypes.c_uint, sz, vp]),
        "bbg_cells_recover": (cint, [vp, vp, sz, vp, ctypes.c_uint, ctypes.c_uint, sz, vp]),
        "bbg_cells_verify_reduce_device": (cint, [vp, vp, ctypes.c_uint, ctypes.c_uint, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp]),
        "bbg_cells_verify_reduce": (cint, [vp, vp, ctypes.c_uint, ctypes.c_uint, vp, sz, vp, vp, sz, vp, vp, vp, vp]),
        "bbg_cells_verify_device": (cint, [vp, vp, vp, ctypes.c_uint, ctypes.c_uint, vp, sz, vp, vp, sz, vp, vp, vp, vp]),
        "bbg_cells_verify": (cint, [vp, vp, vp, ctypes.c_uint, ctypes.c_uint, vp, sz, vp, vp, sz, vp, vp, vp, vp]),
        "bbg_ntt": (cint, [vp, vp, ctypes.c_uint, cint, sz, vp]),
        "bbg_coset_fft_extend": (cint, [vp, vp, ctypes.c_uint, ctypes.c_uint, vp]),
        "bbg_quotient_widget_device": (cint, [vp, cint, vp, ctypes.c_uint, vp, vp, vp]),
        "bbg_poly_linear_combination_device": (cint, [vp, vp, vp, sz, vp, vp, sz]),
        "bbg_permutation_grand_product_device": (cint, [vp, vp, vp, ctypes.c_uint, vp, vp]),
        "bbg_poly_evaluate": (cint, [vp, vp, sz, vp, vp]),
        "bbg_kate_opening": (cint, [vp, vp, vp, sz, vp, vp]),
        "bbg_divide_by_pseudo_vanishing": (cint, [vp, vp, ctypes.c_uint, ctypes.c_uint, sz]),
        "bbg_ntt_device": (cint, [vp, vp, ctypes.c_uint, cint, sz, vp]),
        "bbg_ntt_prepare": (cint, [vp, ctypes.c_uint]),
        "bbg_coset_fft_split": (cint, [vp, vp, ctypes.c_uint, sz]),
        "bbg_coset_fft_split_device": (cint, [vp, vp, ctypes.c_uint, sz]),
        "bbg_scale_powers_device": (cint, [vp, vp, sz, vp, vp]),
        "bbg_fr_root_pow": (cint, [vp, ctypes.c_uint, ctypes.c_uint64, cint, vp]),
        "bbg_fr_pow": (cint, [vp, vp, ctypes.c_uint64, vp]),
        "bbg_cross_dft_device": (cint, [vp, vp, vp, ctypes.c_uint, sz, ctypes.c_uint, cint]),
        "bbg_poly_op_device": (cint, [vp, cint, vp, vp, vp, sz]),
        "bbg_poly_evaluate_device": (cint, [vp, vp, sz, vp, vp]),
        "bbg_kate_opening_device": (cint, [vp, vp, vp, sz, vp, vp]),
        "bbg_divide_by_pseudo_vanishing_device": (cint, [vp, vp, ctypes.c_uint, ctypes.c_uint, sz]),
        "bbg_fr_batch_invert_device": (cint, [vp, vp, vp, sz]),
        "bbg_poly_evaluate_lagrange_device": (cint, [vp, vp, vp, sz, ctypes.c_uint, vp, vp]),
        "bbg_poly_evaluate_lagrange": (cint, [vp, vp, ctypes.c_uint, vp, vp]),
        "bbg_kate_opening_lagrange_device": (cint, [vp, vp, vp, ctypes.c_uint, vp, vp]),
        "bbg_open_points_device": (cint, [vp, vp, ctypes.c_uint, vp, vp, sz, vp, vp]),
        "bbg_open_points": (cint, [vp, vp, ctypes.c_uint, vp, vp, sz, vp, vp]),
        "bbg_open_points_set_budget": (cint, [vp, sz]),
        "bbg_kzg_verify_reduce_device": (cint, [vp, vp, vp, vp, vp, sz, vp, vp, vp]),
        "bbg_kzg_verify_reduce": (cint, [vp, vp, vp, vp, vp, sz, vp, vp]),
        "bbg_kzg_verify_device": (cint, [vp, vp, vp, vp, vp, vp, sz, vp, vp]),
        "bbg_kzg_verify": (cint, [vp, vp, vp, vp, vp, vp, sz, vp, vp]),
        "bbg_wire_sizes": (cint, [cint, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
        "bbg_wire_decode_device": (cint, [vp, cint, vp, sz, vp, vp, vp]),
        "bbg_wire_encode_device": (cint, [vp, cint, vp, sz, cint, vp, vp, vp]),
        "bbg_wire_decode": (cint, [vp, cint, vp, sz, vp, vp, vp]),
        "bbg_wire_encode": (cint, [vp, cint, vp, sz, cint, vp, vp, vp]),
        "bbg_dev_alloc": (cint, [vp, sz, ctypes.POINTER(vp)]),
        "bbg_dev_free": (cint, [vp, vp]),
        "bbg_dev_upload": (cint, [vp, vp, vp, sz]),
        "bbg_dev_download": (cint, [vp, vp, vp, sz]),
        "bbg_set_option": (cint, [vp, ctypes.c_char_p, ctypes.c_long]),
        "bbg_field_op": (cint, [vp, cint, cint, vp, vp, vp, sz]),
        "bbg_limb29_op": (cint, [vp, cint, cint, vp, sz, vp]),
        "bbg_limb29_op_shape": (cint, [cint, cint, ctypes.POINTER(cint), ctypes.POINTER(cint)]),
        "bbg_tower_op": (cint, [vp, cint, vp, sz, vp]),
        "bbg_tower_op_shape": (cint, [cint, ctypes.POINTER(cint), ctypes.POINTER(cint)]),
        "bbg_profile_enable": (cint, [vp, cint]),
        "bbg_profile_get": (cint, [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(sz)]),
        "bbg_prover_create": (cint, [vp, vp, ctypes.c_uint, cint, vp, ctypes.POINTER(vp)]),
        "bbg_prover_create_flavour": (cint, [vp, vp, ctypes.c_uint, cint, vp, ctypes.POINTER(vp)]),
        "bbg_prover_destroy": (None, [vp]),
        "bbg_prover_set_key_poly": (cint, [vp, cint, cint, vp]),
        "bbg_prover_finalize_key": (cint, [vp]),
        "bbg_prover_round1": (cint, [vp, vp, vp]),
        "bbg_prover_round3": (cint, [vp, vp, vp, vp, vp]),
        "bbg_prover_round4": (cint, [vp, vp, vp, vp]),
        "bbg_prover_evaluate": (cint, [vp, sz, vp, vp, vp, vp]),
        "bbg_prover_evaluate_lagrange": (cint, [vp, sz, vp, vp, vp, vp]),
        "bbg_prover_linearise": (cint, [vp, sz, vp, vp, vp, vp]),
        "bbg_prover_round6": (cint, [vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]),
        "bbg_prover_read_poly": (cint, [vp, cint, cint, vp, sz]),
        "bbg_multi_create": (cint, [vp, cint, ctypes.POINTER(vp)]),
        "bbg_multi_destroy": (None, [vp]),
        "bbg_multi_count": (cint, [vp]),
        "bbg_multi_ctx": (vp, [vp, cint]),
        "bbg_multi_sync": (cint, [vp]),
        "bbg_multi_srs_register": (cint, [vp, vp, sz, sz]),
        "bbg_multi_srs_synth_hashed": (cint, [vp, ctypes.c_uint64, sz]),
        "bbg_multi_srs_num_points": (sz, [vp]),
        "bbg_multi_msm": (cint, [vp, vp, sz, sz, vp]),
        "bbg_multi_set_option": (cint, [vp, ctypes.c_char_p, ctypes.c_long]),
        "bbg_multi_ntt_device": (cint, [vp, vp, ctypes.c_uint, cint]),
        "bbg_multi_ntt": (cint, [vp, vp, ctypes.c_uint, cint]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)  # AttributeError here == a symbol declared in bbg.h is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "bbg_device_count", "bbg_init", "bbg_destroy", "bbg_last_error", "bbg_sync", "bbg_join", "bbg_join_lag", "bbg_set_stream", "bbg_srs_register",
    "bbg_srs_register_device", "bbg_srs_synth_linear", "bbg_srs_synth_hashed", "bbg_srs_load_transcript", "bbg_srs_num_points", "bbg_srs_read",
    "bbg_srs_free", "bbg_srs_retain", "bbg_srs_lagrange", "bbg_msm", "bbg_msm_device", "bbg_msm_batch", "bbg_msm_batch_device", "bbg_msm_plan", "bbg_ntt_plan", "bbg_memory_report",
    "bbg_memory_trim", "bbg_prover_device_bytes", "bbg_g1_sum", "bbg_g1_sum_device", "bbg_g1_normalize", "bbg_ntt", "bbg_ntt_device", "bbg_coset_fft_extend", "bbg_quotient_widget_device", "bbg_poly_linear_combination_device", "bbg_permutation_grand_product_device", "bbg_poly_evaluate", "bbg_kate_opening",
    "bbg_divide_by_pseudo_vanishing",
    "bbg_ntt_prepare", "bbg_coset_fft_split", "bbg_coset_fft_split_device", "bbg_scale_powers_device", "bbg_fr_root_pow", "bbg_fr_pow", "bbg_cross_dft_device", "bbg_poly_op_device", "bbg_poly_evaluate_device", "bbg_kate_opening_device",
    "bbg_divide_by_pseudo_vanishing_device", "bbg_dev_alloc", "bbg_dev_free",
    "bbg_dev_upload", "bbg_dev_download", "bbg_set_option", "bbg_field_op", "bbg_limb29_op", "bbg_limb29_op_shape", "bbg_tower_op", "bbg_tower_op_shape", "bbg_profile_enable", "bbg_profile_get",
    "bbg_srs_write_transcript", "bbg_transcript_checksum", "bbg_srs_register_transcript_buffer",
    "bbg_prover_create", "bbg_prover_create_flavour", "bbg_prover_destroy", "bbg_prover_set_key_poly", "bbg_prover_finalize_key", "bbg_prover_round1", "bbg_prover_round3",
    "bbg_prover_round4", "bbg_prover_evaluate", "bbg_prover_linearise", "bbg_prover_round6", "bbg_prover_read_poly",
    "bbg_multi_create", "bbg_multi_destroy", "bbg_multi_count", "bbg_multi_ctx", "bbg_multi_sync", "bbg_multi_srs_register",
    "bbg_multi_srs_synth_hashed", "bbg_multi_srs_num_points", "bbg_multi_msm", "bbg_multi_ntt_device", "bbg_multi_ntt", "bbg_multi_set_option",
    "bbg_g1_fixed_base_mul", "bbg_g1_fixed_base_mul_device", "bbg_srs_synth_powers",
    "bbg_g1_batch_mul", "bbg_g1_batch_mul_device", "bbg_srs_scale_powers",
    "bbg_fr_batch_invert_device", "bbg_poly_evaluate_lagrange_device", "bbg_poly_evaluate_lagrange", "bbg_kate_opening_lagrange_device",
    "bbg_prover_evaluate_lagrange",
    "bbg_g1_ntt", "bbg_g1_ntt_device", "bbg_open_all_prepare", "bbg_open_all_device", "bbg_open_all", "bbg_open_all_device_bytes", "bbg_open_all_free",
    "bbg_open_all_prepare_cells", "bbg_open_all_count",
    "bbg_open_all_batch_reserve", "bbg_open_all_batch_device", "bbg_open_all_batch",
    "bbg_cells_values_device", "bbg_cells_values", "bbg_cells_recover_device", "bbg_cells_recover",
    "bbg_cells_verify_reduce_device", "bbg_cells_verify_reduce", "bbg_cells_verify_device", "bbg_cells_verify",
    "bbg_g1_msm", "bbg_g1_msm_device", "bbg_g1_msm_plan",
    "bbg_g2_mul", "bbg_g2_lines_prepare", "bbg_g2_lines_pairs", "bbg_g2_lines_read", "bbg_g2_lines_free",
    "bbg_pairing_product_device", "bbg_pairing_product", "bbg_pairing_product_wave_device", "bbg_pairing_product_wave",
    "bbg_open_points_device", "bbg_open_points", "bbg_open_points_set_budget",
    "bbg_kzg_verify_reduce_device", "bbg_kzg_verify_reduce", "bbg_kzg_verify_device", "bbg_kzg_verify",
    "bbg_wire_sizes", "bbg_wire_decode_device", "bbg_wire_encode_device", "bbg_wire_decode", "bbg_wire_encode",
]


def wire_sizes(form):
    """(wire bytes, native bytes) per element of a form (bbg_wire_sizes: pure host, no context)."""
    wb, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    if load_library().bbg_wire_sizes(form, ctypes.byref(wb), ctypes.byref(nb)) != 0:
        raise BbgError(f"unknown wire form {form}")
    return wb.value, nb.value


class MemoryInfo(ctypes.Structure):
    """bbg_memory_info (include/bbg.h)."""
    _fields_ = [(k, ctypes.c_size_t) for k in ("srs_points", "srs_tables", "ntt_tables", "msm_arena", "scratch", "prover_keys", "total",
                                               "device_total", "device_free")] + \
               [(k, ctypes.c_uint) for k in ("live_srs", "live_provers", "ntt_domains")]


def _u64(a, shape_last):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim == 1:
        a = a.reshape(-1, shape_last)
    if a.shape[-1] != shape_last:
        raise ValueError(f"expected (*, {shape_last}) uint64 limbs, got {a.shape}")
    return a


class Srs:
    def __init__(self, owner, handle):
        self._owner, self.handle = owner, handle

    @property
    def num_points(self):
        return int(self._owner.lib.bbg_srs_num_points(self.handle))

    def read(self, start=0, count=None):
        count = self.num_points - start if count is None else count
        out = np.empty((count, 8), dtype=np.uint64)
        self._owner._ck(self._owner.lib.bbg_srs_read(self.handle, start, count, out.ctypes.data))
        return out

    def write_transcript(self, directory, points_per_file=0, g2_x_raw=None):
        """Ignition-format files directory/transcriptNN.dat holding points 1 .. n-1 (bbg_srs_write_transcript)."""
        g2 = None if g2_x_raw is None else ctypes.create_string_buffer(bytes(g2_x_raw), 128)
        self._owner._ck(self._owner.lib.bbg_srs_write_transcript(self.handle, str(directory).encode(), points_per_file, g2))

    def lagrange(self, log2n):
        """The Lagrange-base form of the first 2^log2n points, LB[k] = n^-1 sum_j w_n^(-jk) M_j, as an Srs of its own (bbg_srs_lagrange)."""
        h = ctypes.c_void_p()
        self._owner._ck(self._owner.lib.bbg_srs_lagrange(self._owner.ctx, self.handle, log2n, ctypes.byref(h)))
        return Srs(self._owner, h)

    def scale_powers(self, y):
        """The string with P_i' = [y^i] P_i as an Srs of its own; y: Montgomery Fr limbs (bbg_srs_scale_powers)."""
        yy = np.ascontiguousarray(y, dtype=np.uint64).reshape(4)
        h = ctypes.c_void_p()
        self._owner._ck(self._owner.lib.bbg_srs_scale_powers(self._owner.ctx, self.handle, yy.ctypes.data, ctypes.byref(h)))
        return Srs(self._owner, h)

    def free(self):
        if self.handle:
            self._owner.lib.bbg_srs_free(self.handle)
            self.handle = None


class OpenAll:
    """A prepared bbg_open_all handle: all n = 2^log2n opening proofs of a polynomial on its own domain per call, or, prepared with
    log2cell > 0, its n >> log2cell cell proofs (one per coset of 2^log2cell domain points)."""

    def __init__(self, owner, handle, log2n):
        self._owner, self.handle, self.log2n = owner, handle, log2n

    @property
    def count(self):
        """The number of proofs a call writes (bbg_open_all_count)."""
        c = ctypes.c_size_t()
        self._owner._ck(self._owner.lib.bbg_open_all_count(self.handle, ctypes.byref(c)))
        return int(c.value)

    def open(self, coeffs):
        """(count, 8) canonical affine proofs for (n, 4) Montgomery coefficients (bbg_open_all): out[m] = commitment to
        (f(X) - f(w^m)) / (X - w^m), or for a cell handle to the quotient of f by X^l - w^(l m)."""
        c = _u64(coeffs, 4)
        if c.shape[0] != 1 << self.log2n:
            raise ValueError(f"expected {1 << self.log2n} coefficients, got {c.shape[0]}")
        out = np.zeros((self.count, 8), dtype=np.uint64)
        self._owner._ck(self._owner.lib.bbg_open_all(self.handle, c.ctypes.data, out.ctypes.data))
        return out

    def open_device(self, d_coeffs, d_out):
        """Device pointers, d_out of count x 64 B; asynchronous on the context stream (bbg_open_all_device)."""
        self._owner._ck(self._owner.lib.bbg_open_all_device(self.handle, ctypes.c_void_p(d_coeffs), ctypes.c_void_p(d_out)))

    def reserve_batch(self, polys):
        """The batch workspace for `polys` polynomials at a time, at most the library's cap; 0 releases it (bbg_open_all_batch_reserve)."""
        self._owner._ck(self._owner.lib.bbg_open_all_batch_reserve(self.handle, polys))

    def open_batch(self, coeffs):
        """(polys, count, 8) canonical affine proofs for (polys, n, 4) Montgomery coefficients (bbg_open_all_batch): out[p] is what open
        returns for coeffs[p]."""
        c = np.ascontiguousarray(coeffs, dtype=np.uint64)
        if c.ndim != 3 or c.shape[0] < 1 or c.shape[1:] != (1 << self.log2n, 4):
            raise ValueError(f"expected (polys, {1 << self.log2n}, 4) uint64 limbs, got {c.shape}")
        out = np.zeros((c.shape[0], self.count, 8), dtype=np.uint64)
        self._owner._ck(self._owner.lib.bbg_open_all_batch(self.handle, c.ctypes.data, c.shape[0], out.ctypes.data))
        return out

    def open_batch_device(self, d_coeffs, count, d_out):
        """Device pointers: count x n x 32 B in, count x proofs x 64 B out, polynomial-major; asynchronous on the context stream
        (bbg_open_all_batch_device)."""
        self._owner._ck(self._owner.lib.bbg_open_all_batch_device(self.handle, ctypes.c_void_p(d_coeffs), count, ctypes.c_void_p(d_out)))

    def device_bytes(self):
        """The handle's device memory, the batch workspace included while it is reserved (bbg_open_all_device_bytes)."""
        b = ctypes.c_size_t()
        self._owner._ck(self._owner.lib.bbg_open_all_device_bytes(self.handle, ctypes.byref(b)))
        return int(b.value)

    def free(self):
        if self.handle:
            self._owner.lib.bbg_open_all_free(self.handle)
            self.handle = None


class G2Lines:
    """A prepared bbg_g2_lines handle: the line coefficients of `pairs` G2 points, the fixed side of bbg_pairing_product."""

    def __init__(self, owner, handle):
        self._owner, self.handle = owner, handle

    @property
    def pairs(self):
        c = ctypes.c_size_t()
        self._owner._ck(self._owner.lib.bbg_g2_lines_pairs(self.handle, ctypes.byref(c)))
        return int(c.value)

    def read(self, which):
        """The 2088 words (16 704 bytes) of pairing::miller_lines of point `which` (bbg_g2_lines_read)."""
        out = np.zeros(2088, dtype=np.uint64)
        self._owner._ck(self._owner.lib.bbg_g2_lines_read(self.handle, which, out.ctypes.data))
        return out

    def free(self):
        if self.handle:
            self._owner.lib.bbg_g2_lines_free(self.handle)
            self.handle = None


class Bbg:
    """One context per GPU (one process per GPU in multi-GPU runs)."""

    def __init__(self, device=0):
        self.lib = load_library()
        if self.lib.bbg_device_count() <= 0:
            raise BbgError("no HIP device visible: libbbg has no CPU fallback")
        h = ctypes.c_void_p()
        rc = self.lib.bbg_init(device, ctypes.byref(h))
        if rc != 0:
            raise BbgError(f"bbg_init failed ({rc}): {self.lib.bbg_last_error().decode()}")
        self.ctx = h
        self.device = device

    def _ck(self, rc):
        if rc != 0:
            raise BbgError(f"libbbg error {rc}: {self.lib.bbg_last_error().decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.bbg_destroy(self.ctx)
            self.ctx = None

    def sync(self):
        self._ck(self.lib.bbg_sync(self.ctx))

    def join(self, lag=0):
        self._ck(self.lib.bbg_join_lag(self.ctx, lag) if lag else self.lib.bbg_join(self.ctx))

    def set_stream(self, stream_ptr):
        self._ck(self.lib.bbg_set_stream(self.ctx, ctypes.c_void_p(stream_ptr)))

    def set_option(self, key, value):
        self._ck(self.lib.bbg_set_option(self.ctx, key.encode(), int(value)))

    # ---- SRS
    def srs_register(self, points, stride_bytes=64):
        pts = np.ascontiguousarray(points, dtype=np.uint64)
        n = pts.size * 8 // stride_bytes
        h = ctypes.c_void_p()
        self._ck(self.lib.bbg_srs_register(self.ctx, pts.ctypes.data, n, stride_bytes, ctypes.byref(h)))
        return Srs(self, h)

    def srs_register_device(self, d_points, n):
        h = ctypes.c_void_p()
        self._ck(self.lib.bbg_srs_register_device(self.ctx, ctypes.c_void_p(d_points), n, ctypes.byref(h)))
        return Srs(self, h)

    def srs_synth_linear(self, a, s, n):
        h = ctypes.c_void_p()
        self._ck(self.lib.bbg_srs_synth_linear(self.ctx, a, s, n, ctypes.byref(h)))
        return Srs(self, h)

    def srs_synth_hashed(self, seed, n):
        h = ctypes.c_void_p()
        self._ck(self.lib.bbg_srs_synth_hashed(self.ctx, seed, n, ctypes.byref(h)))
        return Srs(self, h)

    def srs_synth_powers(self, x, n):
        """The structured string P_i = [x^i] G, i < n, for a known x (Montgomery Fr limbs) (bbg_srs_synth_powers)."""
        xx = np.ascontiguousarray(x, dtype=np.uint64).reshape(4)
        h = ctypes.c_void_p()
        self._ck(self.lib.bbg_srs_synth_powers(self.ctx, xx.ctypes.data, n, ctypes.byref(h)))
        return Srs(self, h)

    def srs_load_transcript(self, directory, num_points):
        h = ctypes.c_void_p()
        self._ck(self.lib.bbg_srs_load_transcript(self.ctx, str(directory).encode(), num_points, ctypes.byref(h)))
        return Srs(self, h)

    # ---- MSM
    def msm(self, srs, scalars, start=0):
        sc = _u64(scalars, 4)
        out = np.zeros(12, dtype=np.uint64)
        self._ck(self.lib.bbg_msm(self.ctx, srs.handle, sc.ctypes.data, start, sc.shape[0], out.ctypes.data))
        return out

    def msm_device(self, srs, d_scalars, n, d_out, start=0):
        self._ck(self.lib.bbg_msm_device(self.ctx, srs.handle, ctypes.c_void_p(d_scalars), start, n, ctypes.c_void_p(d_out)))

    def msm_batch(self, srs, scalar_list, starts=None):
        """bbg_msm_batch: len(scalar_list) MSMs over one SRS through ONE launch set; returns (count, 12) Jacobians."""
        scs = [_u64(s, 4) for s in scalar_list]
        cnt = len(scs)
        ptrs = (ctypes.c_void_p * cnt)(*[ctypes.c_void_p(s.ctypes.data) for s in scs])
        ns = (ctypes.c_size_t * cnt)(*[s.shape[0] for s in scs])
        fr = None if starts is None else (ctypes.c_size_t * cnt)(*[int(v) for v in starts])
        out = np.zeros((cnt, 12), dtype=np.uint64)
        self._ck(self.lib.bbg_msm_batch(self.ctx, srs.handle, cnt, ptrs, fr, ns, out.ctypes.data))
        return out

    def msm_batch_device(self, srs, d_scalar_ptrs, ns, d_out, starts=None):
        cnt = len(d_scalar_ptrs)
        ptrs = (ctypes.c_void_p * cnt)(*[ctypes.c_void_p(int(p)) for p in d_scalar_ptrs])
        nn = (ctypes.c_size_t * cnt)(*[int(v) for v in ns])
        fr = None if starts is None else (ctypes.c_size_t * cnt)(*[int(v) for v in starts])
        self._ck(self.lib.bbg_msm_batch_device(self.ctx, srs.handle, cnt, ptrs, fr, nn, ctypes.c_void_p(d_out)))

    def ntt_plan(self, log2n):
        """{passes, log_radix, kernel, tile_log} of a 2^log2n transform as it would run now (bbg_ntt_plan)."""
        cint = ctypes.c_int
        passes, kernel, tile = cint(), cint(), cint()
        radix = (cint * 4)()
        self._ck(self.lib.bbg_ntt_plan(self.ctx, log2n, ctypes.byref(passes), radix, ctypes.byref(kernel), ctypes.byref(tile)))
        names = {0: "k_ntt_pass", 8: "k_ntt_pass8", 81: "k_ntt_pass8s", 29: "k_ntt_pass29"}
        return {"passes": passes.value, "log_radix": [radix[q] for q in range(passes.value)], "kernel": names.get(kernel.value, str(kernel.value)),
                "tile_log": tile.value}

    def msm_plan(self, n, srs=None):
        """(window bits C, windows) an n-term MSM would run with now (bbg_msm_plan)."""
        c, w = ctypes.c_int(), ctypes.c_int()
        self._ck(self.lib.bbg_msm_plan(self.ctx, srs.handle if srs is not None else None, n, ctypes.byref(c), ctypes.byref(w)))
        return c.value, w.value

    def memory_report(self):
        """bbg_memory_report as a dict (bytes by purpose, live handle counts, hipMemGetInfo)."""
        info = MemoryInfo()
        self._ck(self.lib.bbg_memory_report(self.ctx, ctypes.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in MemoryInfo._fields_}

    def memory_trim(self, tables=False):
        rel = ctypes.c_size_t()
        self._ck(self.lib.bbg_memory_trim(self.ctx, 1 if tables else 0, ctypes.byref(rel)))
        return int(rel.value)

    def g1_sum(self, jacobians):
        j = _u64(jacobians, 12)
        out = np.zeros(12, dtype=np.uint64)
        self._ck(self.lib.bbg_g1_sum(self.ctx, j.ctypes.data, j.shape[0], out.ctypes.data))
        return out

    def g1_sum_device(self, d_jacobians, n, d_out):
        self._ck(self.lib.bbg_g1_sum_device(self.ctx, ctypes.c_void_p(d_jacobians), n, ctypes.c_void_p(d_out)))

    def g1_normalize(self, jacobians):
        j = _u64(jacobians, 12)
        out = np.zeros((j.shape[0], 8), dtype=np.uint64)
        self._ck(self.lib.bbg_g1_normalize(self.ctx, j.ctypes.data, j.shape[0], out.ctypes.data))
        return out

    def g1_fixed_base_mul(self, scalars, base=None):
        """scalars[i] * base as (n, 8) canonical affine points; base = one affine point (8 limbs), None = the generator
        (bbg_g1_fixed_base_mul)."""
        sc = _u64(scalars, 4)
        b = None if base is None else np.ascontiguousarray(base, dtype=np.uint64).reshape(8)
        out = np.zeros((sc.shape[0], 8), dtype=np.uint64)
        self._ck(self.lib.bbg_g1_fixed_base_mul(self.ctx, None if b is None else b.ctypes.data, sc.ctypes.data, sc.shape[0], out.ctypes.data))
        return out

    def g1_fixed_base_mul_device(self, d_scalars, n, d_out, base=None):
        b = None if base is None else np.ascontiguousarray(base, dtype=np.uint64).reshape(8)
        self._ck(self.lib.bbg_g1_fixed_base_mul_device(self.ctx, None if b is None else b.ctypes.data, ctypes.c_void_p(d_scalars), n,
                                                       ctypes.c_void_p(d_out)))

    def g1_batch_mul(self, points, scalars, one_scalar=False):
        """scalars[i] * points[i] (one_scalar: scalars[0] * points[i]) as (n, 8) canonical affine points (bbg_g1_batch_mul)."""
        pt, sc = _u64(points, 8), _u64(scalars, 4)
        if sc.shape[0] != (1 if one_scalar else pt.shape[0]):
            raise ValueError("one scalar per point, or exactly one with one_scalar")
        out = np.zeros((pt.shape[0], 8), dtype=np.uint64)
        self._ck(self.lib.bbg_g1_batch_mul(self.ctx, pt.ctypes.data, sc.ctypes.data, pt.shape[0], int(bool(one_scalar)), out.ctypes.data))
        return out

    def g1_batch_mul_device(self, d_points, d_scalars, n, d_out, one_scalar=False):
        self._ck(self.lib.bbg_g1_batch_mul_device(self.ctx, ctypes.c_void_p(d_points), ctypes.c_void_p(d_scalars), n, int(bool(one_scalar)),
                                                  ctypes.c_void_p(d_out)))

    def g1_msm(self, points, scalars, window_bits=0):
        """sum_i scalars[i] * points[i] over plain (n, 8) affine points, no SRS: one canonical affine point (8 limbs), the affine encoding
        of infinity for an infinite sum and for n = 0; window_bits 0 = automatic, else 2 .. 16 (bbg_g1_msm)."""
        pt, sc = _u64(points, 8), _u64(scalars, 4)
        if sc.shape[0] != pt.shape[0]:
            raise ValueError("one scalar per point")
        out = np.zeros(8, dtype=np.uint64)
        self._ck(self.lib.bbg_g1_msm(self.ctx, pt.ctypes.data, sc.ctypes.data, pt.shape[0], int(window_bits), out.ctypes.data))
        return out

    def g1_msm_device(self, d_points, d_scalars, n, d_out, window_bits=0):
        """Device pointers, 64 bytes at d_out; asynchronous (bbg_g1_msm_device)."""
        self._ck(self.lib.bbg_g1_msm_device(self.ctx, ctypes.c_void_p(d_points), ctypes.c_void_p(d_scalars), n, int(window_bits), ctypes.c_void_p(d_out)))

    @staticmethod
    def g1_msm_plan(n, window_bits=0):
        """(c, windows, chunk_terms, segment_entries) of a bbg_g1_msm call with these arguments; needs no device and no context
        (bbg_g1_msm_plan)."""
        c, windows, chunk, seg = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        lib = load_library()
        if lib.bbg_g1_msm_plan(n, int(window_bits), ctypes.byref(c), ctypes.byref(windows), ctypes.byref(chunk), ctypes.byref(seg)) != 0:
            raise BbgError(lib.bbg_last_error().decode())
        return c.value, windows.value, chunk.value, seg.value

    # ---- G2 and pairing product checks (csrc/pairing.hip)
    def g2_mul(self, scalars, base=None):
        """scalars[i] * base on the twist as (n, 16) canonical affine points x | y; base = one point (16 limbs), None = the generator of G2;
        infinity in the affine encoding applied to x.c0 (bbg_g2_mul)."""
        sc = _u64(scalars, 4)
        b = None if base is None else np.ascontiguousarray(base, dtype=np.uint64).reshape(16)
        out = np.zeros((sc.shape[0], 16), dtype=np.uint64)
        self._ck(self.lib.bbg_g2_mul(self.ctx, None if b is None else b.ctypes.data, sc.ctypes.data, sc.shape[0], out.ctypes.data))
        return out

    def g2_lines_prepare(self, g2_points):
        """A G2Lines for (pairs, 16) finite points of the order-r subgroup of the twist, 1 <= pairs <= 8 (bbg_g2_lines_prepare)."""
        q = _u64(g2_points, 16)
        h = ctypes.c_void_p()
        self._ck(self.lib.bbg_g2_lines_prepare(self.ctx, q.ctypes.data, q.shape[0], ctypes.byref(h)))
        return G2Lines(self, h)

    def pairing_product(self, lines, g1_points, want_values=True):
        """(values, status) of count products over (count * pairs, 8) affine G1 points, product i pairing point i pairs + j with point j of
        `lines`: values (count, 48) canonical fq12 words (None without want_values), status (count,) uint32 with 1 = the product is one,
        0 = it is not.  A G1 point off the curve raises BbgError (bbg_pairing_product)."""
        p = _u64(g1_points, 8)
        count, rest = divmod(p.shape[0], lines.pairs)
        if rest:
            raise ValueError(f"expected a multiple of {lines.pairs} points, got {p.shape[0]}")
        values = np.zeros((count, 48), dtype=np.uint64) if want_values else None
        status = np.zeros(count, dtype=np.uint32)
        self._ck(self.lib.bbg_pairing_product(self.ctx, lines.handle, p.ctypes.data, count, None if values is None else values.ctypes.data, status.ctypes.data))
        return values, status

    def pairing_product_device(self, lines, d_g1_points, count, d_out_fq12=None, d_status=None):
        """Device pointers (count x pairs x 64 B in; count x 384 B and count x 4 B out, either may be None); asynchronous on the context
        stream (bbg_pairing_product_device)."""
        self._ck(self.lib.bbg_pairing_product_device(self.ctx, lines.handle, ctypes.c_void_p(d_g1_points), count,
                                                     ctypes.c_void_p(d_out_fq12) if d_out_fq12 else None, ctypes.c_void_p(d_status) if d_status else None))

    def pairing_product_wave(self, lines, g1_points, want_values=True):
        """pairing_product with one wave per product instead of one lane: the same (values, status), bit for bit; the form for a few
        products, where latency counts (bbg_pairing_product_wave)."""
        p = _u64(g1_points, 8)
        count, rest = divmod(p.shape[0], lines.pairs)
        if rest:
            raise ValueError(f"expected a multiple of {lines.pairs} points, got {p.shape[0]}")
        values = np.zeros((count, 48), dtype=np.uint64) if want_values else None
        status = np.zeros(count, dtype=np.uint32)
        self._ck(self.lib.bbg_pairing_product_wave(self.ctx, lines.handle, p.ctypes.data, count, None if values is None else values.ctypes.data,
                                                   status.ctypes.data))
        return values, status

    def pairing_product_wave_device(self, lines, d_g1_points, count, d_out_fq12=None, d_status=None):
        """Device pointers as pairing_product_device; asynchronous on the context stream, no working memory
        (bbg_pairing_product_wave_device)."""
        self._ck(self.lib.bbg_pairing_product_wave_device(self.ctx, lines.handle, ctypes.c_void_p(d_g1_points), count,
                                                          ctypes.c_void_p(d_out_fq12) if d_out_fq12 else None, ctypes.c_void_p(d_status) if d_status else None))

    def g1_ntt(self, points, inverse=False):
        """The NTT over G1 of (n, 8) affine points, n a power of two >= 2: out[k] = sum_j w^(jk) P_j, or n^-1 sum_j w^(-jk) P_j with
        inverse; canonical affine, infinite outputs in the affine encoding of infinity (bbg_g1_ntt)."""
        pt = _u64(points, 8)
        n = pt.shape[0]
        log2n = n.bit_length() - 1
        if n == 0 or (1 << log2n) != n:
            raise ValueError("G1 NTT size must be a power of two")
        out = np.zeros((n, 8), dtype=np.uint64)
        self._ck(self.lib.bbg_g1_ntt(self.ctx, pt.ctypes.data, log2n, int(bool(inverse)), out.ctypes.data))
        return out

    def g1_ntt_device(self, d_points, log2n, d_out, inverse=False):
        """Device pointers, d_out may be d_points; asynchronous (bbg_g1_ntt_device)."""
        self._ck(self.lib.bbg_g1_ntt_device(self.ctx, ctypes.c_void_p(d_points), log2n, int(bool(inverse)), ctypes.c_void_p(d_out)))

    def open_all_prepare(self, srs, log2n, log2cell=0):
        """An OpenAll for polynomials of 2^log2n coefficients over the first 2^log2n - 1 points of srs (bbg_open_all_prepare); with
        log2cell > 0 one that proves cells of 2^log2cell points (bbg_open_all_prepare_cells)."""
        h = ctypes.c_void_p()
        if log2cell == 0:
            self._ck(self.lib.bbg_open_all_prepare(self.ctx, srs.handle, log2n, ctypes.byref(h)))
        else:
            self._ck(self.lib.bbg_open_all_prepare_cells(self.ctx, srs.handle, log2n, log2cell, ctypes.byref(h)))
        return OpenAll(self, h, log2n)

    # ---- cells as data (csrc/cells.hip): n = 2^log2n, l = 2^log2cell, r = n / l, cell m = { w^(m + r t) : t < l }
    def cells_values(self, coeffs, log2n, log2cell):
        """The values of every cell of (count * n, 4) Montgomery coefficients, count polynomials one after the other: (count * n, 4)
        canonical words, out[p n + m l + t] = f_p(w^(m + r t)) (bbg_cells_values)."""
        c = _u64(coeffs, 4)
        count, rest = divmod(c.shape[0], 1 << log2n)
        if rest:
            raise ValueError(f"expected a multiple of {1 << log2n} coefficients, got {c.shape[0]}")
        out = np.zeros_like(c)
        self._ck(self.lib.bbg_cells_values(self.ctx, c.ctypes.data, log2n, log2cell, count, out.ctypes.data))
        return out

    def cells_values_device(self, d_coeffs, log2n, log2cell, count, d_out):
        """Device pointers, count x n values each, no overlap; asynchronous on the context stream (bbg_cells_values_device)."""
        self._ck(self.lib.bbg_cells_values_device(self.ctx, ctypes.c_void_p(d_coeffs), log2n, log2cell, count, ctypes.c_void_p(d_out)))

    def cells_recover(self, cell_ids, values, log2n, log2cell):
        """The coefficients of the polynomials of degree < K l through the K cells cell_ids: values is (count * K * l, 4), cell k of
        polynomial p at (p K + k) l; returns (count * n, 4) canonical words (bbg_cells_recover)."""
        ids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        v = _u64(values, 4)
        per = max(ids.shape[0], 1) << log2cell
        count, rest = divmod(v.shape[0], per)
        if rest:
            raise ValueError(f"expected a multiple of {per} values, got {v.shape[0]}")
        out = np.zeros((count << log2n, 4), dtype=np.uint64)
        self._ck(self.lib.bbg_cells_recover(self.ctx, ids.ctypes.data, ids.shape[0], v.ctypes.data, log2n, log2cell, count, out.ctypes.data))
        return out

    def cells_recover_device(self, cell_ids, d_values, log2n, log2cell, count, d_out_coeffs):
        """Device pointers (count x K x l values in, count x n coefficients out, no overlap), cell_ids on the host; asynchronous
        (bbg_cells_recover_device)."""
        ids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        self._ck(self.lib.bbg_cells_recover_device(self.ctx, ids.ctypes.data, ids.shape[0], ctypes.c_void_p(d_values), log2n, log2cell, count,
                                                   ctypes.c_void_p(d_out_coeffs)))

    # ---- a batch of cell proofs reduced to the two points of one pairing check (csrc/cells_verify.hip)
    def cells_verify_reduce(self, srs, log2n, log2cell, commitments, commitment_ids, cell_ids, values, proofs, rho):
        """K cells: cell k has commitment commitments[commitment_ids[k]], cell index cell_ids[k], the l values values[k l : (k + 1) l] and the
        proof proofs[k].  Returns (2, 8) canonical affine words (L, R): every proof is valid iff e(L, [x^l]_2) = e(R, [1]_2), up to the choice
        of rho (4 Montgomery words).  A point off the curve raises BbgError (bbg_cells_verify_reduce)."""
        com, prf, v = _u64(commitments, 8), _u64(proofs, 8), _u64(values, 4)
        cids = np.ascontiguousarray(commitment_ids, dtype=np.uint32).reshape(-1)
        mids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        K = mids.shape[0]
        if cids.shape[0] != K or prf.shape[0] != K or v.shape[0] != K << log2cell:
            raise ValueError(f"expected {K} commitment ids and proofs and {K << log2cell} values")
        rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(4)
        out = np.zeros((2, 8), dtype=np.uint64)
        self._ck(self.lib.bbg_cells_verify_reduce(self.ctx, srs.handle, log2n, log2cell, com.ctypes.data, com.shape[0], cids.ctypes.data, mids.ctypes.data, K,
                                                  v.ctypes.data, prf.ctypes.data, rho.ctypes.data, out.ctypes.data))
        return out

    def cells_verify_reduce_device(self, srs, log2n, log2cell, d_commitments, ncom, commitment_ids, cell_ids, d_values, d_proofs, rho, d_out,
                                   d_off_curve=None):
        """Device pointers (ncom x 64 B, K x l x 32 B, K x 64 B in; 128 B and, optionally, one uint32 out), the ids and rho on the host;
        asynchronous on the context stream (bbg_cells_verify_reduce_device)."""
        cids = np.ascontiguousarray(commitment_ids, dtype=np.uint32).reshape(-1)
        mids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        if cids.shape[0] != mids.shape[0]:
            raise ValueError("one commitment id and one cell id per cell")
        rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(4)
        self._ck(self.lib.bbg_cells_verify_reduce_device(self.ctx, srs.handle, log2n, log2cell, ctypes.c_void_p(d_commitments), ncom, cids.ctypes.data,
                                                         mids.ctypes.data, mids.shape[0], ctypes.c_void_p(d_values), ctypes.c_void_p(d_proofs),
                                                         rho.ctypes.data, ctypes.c_void_p(d_out), ctypes.c_void_p(d_off_curve) if d_off_curve else None))

    def cells_verify(self, srs, lines, log2n, log2cell, commitments, commitment_ids, cell_ids, values, proofs, rho):
        """The verdict on K cells (arguments as cells_verify_reduce) against `lines`, the G2Lines of ([x^l]_2, [1]_2): 1 = every proof is
        valid under rho, 0 = not.  A point off the curve (status 2) raises BbgError (bbg_cells_verify)."""
        com, prf, v = _u64(commitments, 8), _u64(proofs, 8), _u64(values, 4)
        cids = np.ascontiguousarray(commitment_ids, dtype=np.uint32).reshape(-1)
        mids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        K = mids.shape[0]
        if cids.shape[0] != K or prf.shape[0] != K or v.shape[0] != K << log2cell:
            raise ValueError(f"expected {K} commitment ids and proofs and {K << log2cell} values")
        rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(4)
        status = ctypes.c_uint32(0)
        self._ck(self.lib.bbg_cells_verify(self.ctx, srs.handle, lines.handle, log2n, log2cell, com.ctypes.data, com.shape[0], cids.ctypes.data, mids.ctypes.data,
                                           K, v.ctypes.data, prf.ctypes.data, rho.ctypes.data, ctypes.byref(status)))
        return int(status.value)

    def cells_verify_device(self, srs, lines, log2n, log2cell, d_commitments, ncom, commitment_ids, cell_ids, d_values, d_proofs, rho, d_status):
        """Device pointers as cells_verify_reduce_device, d_status one uint32 (1 / 0 / 2); the ids and rho on the host; asynchronous on the
        context stream (bbg_cells_verify_device)."""
        cids = np.ascontiguousarray(commitment_ids, dtype=np.uint32).reshape(-1)
        mids = np.ascontiguousarray(cell_ids, dtype=np.uint32).reshape(-1)
        if cids.shape[0] != mids.shape[0]:
            raise ValueError("one commitment id and one cell id per cell")
        rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(4)
        self._ck(self.lib.bbg_cells_verify_device(self.ctx, srs.handle, lines.handle, log2n, log2cell, ctypes.c_void_p(d_commitments), ncom, cids.ctypes.data,
                                                  mids.ctypes.data, mids.shape[0], ctypes.c_void_p(d_values), ctypes.c_void_p(d_proofs), rho.ctypes.data,
                                                  ctypes.c_void_p(d_status)))

    # ---- NTT
    def ntt(self, coeffs, op=FFT, generator_size=0, constant=None):
        a = _u64(coeffs, 4).copy()
        n = a.shape[0]
        log2n = n.bit_length() - 1
        if n == 0 or (1 << log2n) != n:
            raise ValueError("NTT size must be a power of two")
        c = None if constant is None else np.ascontiguousarray(constant, dtype=np.uint64)
        self._ck(self.lib.bbg_ntt(self.ctx, a.ctypes.data, log2n, op, generator_size, None if c is None else c.ctypes.data))
        return a

    def coset_fft_extend(self, coeffs, log2_domain):
        """The prover's FFT work item (work_queue.hpp:252-264): n coefficients -> 2^log2_domain + 4 coset evaluations."""
        a = _u64(coeffs, 4)
        n = a.shape[0]
        log2n = n.bit_length() - 1
        if n == 0 or (1 << log2n) != n:
            raise ValueError("coefficient count must be a power of two")
        out = np.empty(((1 << log2_domain) + 4, 4), dtype=np.uint64)
        self._ck(self.lib.bbg_coset_fft_extend(self.ctx, a.ctypes.data, log2n, log2_domain, out.ctypes.data))
        return out

    def poly_linear_combination_device(self, d_polys, scalars, d_base, d_out, n):
        """out = base + sum_k polys[k] * scalars[k] (d_base may be 0/None)."""
        arr = (ctypes.c_void_p * max(len(d_polys), 1))(*[ctypes.c_void_p(int(p)) for p in d_polys])
        sc = _u64(scalars, 4) if len(d_polys) else np.zeros((1, 4), dtype=np.uint64)
        self._ck(self.lib.bbg_poly_linear_combination_device(self.ctx, arr, sc.ctypes.data, len(d_polys),
                                                             ctypes.c_void_p(d_base) if d_base else None, ctypes.c_void_p(d_out), n))

    def permutation_grand_product_device(self, d_wires, d_sigmas, log2n, beta, gamma, ks, d_z):
        w = (ctypes.c_void_p * 4)(*[ctypes.c_void_p(int(p)) for p in d_wires])
        s_ = (ctypes.c_void_p * 4)(*[ctypes.c_void_p(int(p)) for p in d_sigmas])
        ch = np.ascontiguousarray(np.concatenate([np.reshape(beta, (1, 4)), np.reshape(gamma, (1, 4)), np.reshape(ks, (3, 4))]), dtype=np.uint64)
        self._ck(self.lib.bbg_permutation_grand_product_device(self.ctx, w, s_, log2n, ch.ctypes.data, ctypes.c_void_p(d_z)))

    def quotient_widget_device(self, widget, d_polys, log2_large, challenges, d_quotient):
        """d_polys: list of BBG_QP_COUNT device addresses (0 = not supplied), BBG_QP_EXT_COUNT = 23 for the MiMC widget (7);
        challenges: (9, 4) uint64.  Returns the next alpha_base."""
        padded = list(d_polys) + [0] * max(0, 23 - len(d_polys))  # the library may read the extended table: never hand it a short array
        arr = (ctypes.c_void_p * len(padded))(*[ctypes.c_void_p(int(p)) if p else None for p in padded])
        ch = np.ascontiguousarray(challenges, dtype=np.uint64)
        assert ch.shape == (9, 4)
        out = np.zeros(4, dtype=np.uint64)
        self._ck(self.lib.bbg_quotient_widget_device(self.ctx, widget, arr, log2_large, ch.ctypes.data, ctypes.c_void_p(d_quotient),
                                                     out.ctypes.data))
        return out

    def ntt_device(self, d_coeffs, log2n, op=FFT, generator_size=0, constant=None):
        c = None if constant is None else np.ascontiguousarray(constant, dtype=np.uint64)
        self._ck(self.lib.bbg_ntt_device(self.ctx, ctypes.c_void_p(d_coeffs), log2n, op, generator_size,
                                         None if c is None else c.ctypes.data))

    def ntt_prepare(self, log2n):
        self._ck(self.lib.bbg_ntt_prepare(self.ctx, log2n))

    def coset_fft_split(self, coeffs, ext):
        a = _u64(coeffs, 4)
        n = a.shape[0]
        log2n = n.bit_length() - 1
        buf = np.zeros((n * ext, 4), dtype=np.uint64)
        buf[:n] = a
        self._ck(self.lib.bbg_coset_fft_split(self.ctx, buf.ctypes.data, log2n, ext))
        return buf

    # ---- sharded-NTT building blocks
    def scale_powers_device(self, d_a, count, base, start=None):
        b = np.ascontiguousarray(base, dtype=np.uint64)
        s_ = None if start is None else np.ascontiguousarray(start, dtype=np.uint64)
        self._ck(self.lib.bbg_scale_powers_device(self.ctx, ctypes.c_void_p(d_a), count, None if s_ is None else s_.ctypes.data,
                                                  b.ctypes.data))

    def fr_root_pow(self, log2n, e, inverse=False):
        out = np.zeros(4, dtype=np.uint64)
        self._ck(self.lib.bbg_fr_root_pow(self.ctx, log2n, e, 1 if inverse else 0, out.ctypes.data))
        return out

    def fr_pow(self, base, e):
        b = np.ascontiguousarray(base, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        self._ck(self.lib.bbg_fr_pow(self.ctx, b.ctypes.data, e, out.ctypes.data))
        return out

    def cross_dft_device(self, d_in, d_out, log2g, length, log2n, inverse=False):
        self._ck(self.lib.bbg_cross_dft_device(self.ctx, ctypes.c_void_p(d_in), ctypes.c_void_p(d_out), log2g, length, log2n,
                                               1 if inverse else 0))

    # ---- polynomial helpers (device pointers)
    def poly_op_device(self, op, d_a, d_b, d_r, n):
        self._ck(self.lib.bbg_poly_op_device(self.ctx, op, ctypes.c_void_p(d_a), ctypes.c_void_p(d_b), ctypes.c_void_p(d_r), n))

    def poly_evaluate_device(self, d_coeffs, n, z):
        zz = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        self._ck(self.lib.bbg_poly_evaluate_device(self.ctx, ctypes.c_void_p(d_coeffs), n, zz.ctypes.data, out.ctypes.data))
        return out

    def kate_opening_device(self, d_src, d_dest, n, z):
        zz = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        self._ck(self.lib.bbg_kate_opening_device(self.ctx, ctypes.c_void_p(d_src), ctypes.c_void_p(d_dest), n, zz.ctypes.data,
                                                  out.ctypes.data))
        return out

    # ---- Lagrange form: values on the 2^log2n domain instead of coefficients (csrc/barycentric.hip)
    def fr_batch_invert_device(self, d_in, d_out, n):
        """out[i] = in[i]^-1, zero stays zero; d_out may be d_in.  Asynchronous."""
        self._ck(self.lib.bbg_fr_batch_invert_device(self.ctx, ctypes.c_void_p(d_in), ctypes.c_void_p(d_out), n))

    def poly_evaluate_lagrange_device(self, d_evals, log2n, z, shifted=None):
        """F_k(z), or F_k(z * w) where shifted[k], for the device arrays d_evals[k] of 2^log2n values: (count, 4) canonical words."""
        count = len(d_evals)
        arr = (ctypes.c_void_p * max(count, 1))(*[ctypes.c_void_p(int(p)) for p in d_evals])
        sh = None if shifted is None else (ctypes.c_int * max(count, 1))(*[int(bool(x)) for x in shifted])
        zz = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros((max(count, 1), 4), dtype=np.uint64)
        self._ck(self.lib.bbg_poly_evaluate_lagrange_device(self.ctx, arr, sh, count, log2n, zz.ctypes.data, out.ctypes.data))
        return out[:count]

    def poly_evaluate_lagrange(self, evals, z):
        """Host-buffer form for one polynomial of 2^k values."""
        a = _u64(evals, 4)
        n = a.shape[0]
        log2n = n.bit_length() - 1
        if n == 0 or (1 << log2n) != n:
            raise ValueError("value count must be a power of two")
        zz = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        self._ck(self.lib.bbg_poly_evaluate_lagrange(self.ctx, a.ctypes.data, log2n, zz.ctypes.data, out.ctypes.data))
        return out

    def kate_opening_lagrange_device(self, d_evals, d_dest, log2n, z):
        """d_dest = the values of (F(X) - F(z)) / (X - z) on the domain; returns F(z)."""
        zz = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        self._ck(self.lib.bbg_kate_opening_lagrange_device(self.ctx, ctypes.c_void_p(d_evals), ctypes.c_void_p(d_dest), log2n, zz.ctypes.data,
                                                           out.ctypes.data))
        return out

    # ---- many Lagrange-form polynomials, each opened at its own point (csrc/open_points.hip)
    def open_points(self, lagrange, evals, z, proofs=True):
        """(y, proofs) for (count, n, 4) Montgomery values and (count, 4) points: y[k] = F_k(z[k]) as (count, 4) canonical words and
        proofs[k] = the commitment over `lagrange` (an Srs in Lagrange form) to (F_k(X) - y[k]) / (X - z[k]) as (count, 8) canonical affine
        words.  proofs=False evaluates only: `lagrange` may be None and the second result is None (bbg_open_points)."""
        e = np.ascontiguousarray(evals, dtype=np.uint64)
        if e.ndim != 3 or e.shape[0] < 1 or e.shape[2] != 4 or e.shape[1] & (e.shape[1] - 1) or e.shape[1] < 2:
            raise ValueError(f"expected (count, 2^k, 4) uint64 limbs, got {e.shape}")
        zz = _u64(z, 4)
        if zz.shape[0] != e.shape[0]:
            raise ValueError("one point per polynomial")
        count, log2n = e.shape[0], e.shape[1].bit_length() - 1
        y = np.zeros((count, 4), dtype=np.uint64)
        out = np.zeros((count, 8), dtype=np.uint64) if proofs else None
        self._ck(self.lib.bbg_open_points(self.ctx, lagrange.handle if lagrange is not None else None, log2n, e.ctypes.data, zz.ctypes.data, count,
                                          y.ctypes.data, out.ctypes.data if proofs else None))
        return y, out

    def open_points_device(self, lagrange, log2n, d_evals, d_z, count, d_y, d_proofs=None):
        """Device pointers: count x n x 32 B values and count x 32 B points in, count x 32 B values and (unless None) count x 64 B proofs
        out; asynchronous on the context stream (bbg_open_points_device)."""
        self._ck(self.lib.bbg_open_points_device(self.ctx, lagrange.handle if lagrange is not None else None, log2n, ctypes.c_void_p(d_evals),
                                                 ctypes.c_void_p(d_z), count, ctypes.c_void_p(d_y), ctypes.c_void_p(d_proofs) if d_proofs else None))

    def open_points_set_budget(self, nbytes):
        """The bytes a chunk of open_points may take of working memory; 0 = the default of 1 GiB (bbg_open_points_set_budget)."""
        self._ck(self.lib.bbg_open_points_set_budget(self.ctx, int(nbytes)))

    # ---- openings at arbitrary points reduced to the two points of one pairing check (csrc/kzg_verify.hip)
    def kzg_verify_reduce(self, commitments, z, y, proofs, rho):
        """N openings (commitments[i], z[i], y[i], proofs[i]): (2, 8) canonical affine words (L, R); every opening is valid iff
        e(L, [x]_2) = e(R, [1]_2), up to the choice of rho (4 Montgomery words).  A point off the curve raises BbgError
        (bbg_kzg_verify_reduce)."""
        com, prf, zz, yy = _u64(commitments, 8), _u64(proofs, 8), _u64(z, 4), _u64(y, 4)
        N = com.shape[0]
        if prf.shape[0] != N or zz.shape[0] != N or yy.shape[0] != N:
            raise ValueError(f"expected {N} points, values and proofs")
        rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(4)
        out = np.zeros((2, 8), dtype=np.uint64)
        self._ck(self.lib.bbg_kzg_verify_reduce(self.ctx, com.ctypes.data, zz.ctypes.data, yy.ctypes.data, prf.ctypes.data, N, rho.ctypes.data, out.ctypes.data))
        return out

    def kzg_verify_reduce_device(self, d_commitments, d_z, d_y, d_proofs, N, rho, d_out, d_off_curve=None):
        """Device pointers (N x 64 B, N x 32 B, N x 32 B, N x 64 B in; 128 B and, optionally, one uint32 out), rho on the host; asynchronous on
        the context stream (bbg_kzg_verify_reduce_device)."""
        rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(4)
        self._ck(self.lib.bbg_kzg_verify_reduce_device(self.ctx, ctypes.c_void_p(d_commitments), ctypes.c_void_p(d_z), ctypes.c_void_p(d_y),
                                                       ctypes.c_void_p(d_proofs), N, rho.ctypes.data, ctypes.c_void_p(d_out),
                                                       ctypes.c_void_p(d_off_curve) if d_off_curve else None))

    def kzg_verify(self, lines, commitments, z, y, proofs, rho):
        """The verdict on N openings (arguments as kzg_verify_reduce) against `lines`, the G2Lines of ([x]_2, [1]_2): 1 = every opening is
        valid under rho, 0 = not.  A point off the curve (status 2) raises BbgError (bbg_kzg_verify)."""
        com, prf, zz, yy = _u64(commitments, 8), _u64(proofs, 8), _u64(z, 4), _u64(y, 4)
        N = com.shape[0]
        if prf.shape[0] != N or zz.shape[0] != N or yy.shape[0] != N:
            raise ValueError(f"expected {N} points, values and proofs")
        rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(4)
        status = ctypes.c_uint32(0)
        self._ck(self.lib.bbg_kzg_verify(self.ctx, lines.handle, com.ctypes.data, zz.ctypes.data, yy.ctypes.data, prf.ctypes.data, N, rho.ctypes.data,
                                         ctypes.byref(status)))
        return int(status.value)

    def kzg_verify_device(self, lines, d_commitments, d_z, d_y, d_proofs, N, rho, d_status):
        """Device pointers as kzg_verify_reduce_device, d_status one uint32 (1 / 0 / 2); rho on the host; asynchronous on the context stream
        (bbg_kzg_verify_device)."""
        rho = np.ascontiguousarray(rho, dtype=np.uint64).reshape(4)
        self._ck(self.lib.bbg_kzg_verify_device(self.ctx, lines.handle, ctypes.c_void_p(d_commitments), ctypes.c_void_p(d_z), ctypes.c_void_p(d_y),
                                                ctypes.c_void_p(d_proofs), N, rho.ctypes.data, ctypes.c_void_p(d_status)))

    # ---- wire forms of G1 points and scalars (csrc/wire.hip)
    def _wire_host(self, fn, form, src, n, out, extra, strict):
        status = np.zeros(n, dtype=np.uint32)
        bad = ctypes.c_uint32(0)
        rc = fn(self.ctx, form, src.ctypes.data, n, *extra, out.ctypes.data, status.ctypes.data, ctypes.byref(bad))
        if rc != 0 and (strict or bad.value == 0):  # a bad element returns BBG_E_INVALID behind the outputs; anything else left them untouched
            self._ck(rc)
        return out, status, int(bad.value)

    def wire_decode(self, form, wire, strict=True):
        """n wire elements (bytes, or any array of n x wire_sizes(form)[0] bytes) to (native, status, bad): native (n, 8) Montgomery affine or
        (n, 4) Montgomery Fr words, status (n,) uint32 (1 valid, 3 infinity, 0 malformed, 2 not on the curve), bad the count of 0s and 2s.
        strict: a bad element raises BbgError; strict=False returns what the call wrote (bbg_wire_decode)."""
        wb, nb = wire_sizes(form)
        src = np.frombuffer(wire, dtype=np.uint8) if isinstance(wire, (bytes, bytearray)) else np.ascontiguousarray(wire).view(np.uint8).reshape(-1)
        if src.size % wb:
            raise ValueError(f"expected a multiple of {wb} bytes, got {src.size}")
        n = src.size // wb
        return self._wire_host(self.lib.bbg_wire_decode, form, src, n, np.zeros((n, nb // 8), dtype=np.uint64), (), strict)

    def wire_encode(self, form, native, check=1, strict=True):
        """The inverse: native words to (wire, status, bad), wire an (n, wire_sizes(form)[0]) uint8 array.  check = 1 tests every finite point
        against the curve (status 2, counted in bad, the form's infinity written) (bbg_wire_encode)."""
        wb, nb = wire_sizes(form)
        src = _u64(native, nb // 8)
        n = src.shape[0]
        return self._wire_host(self.lib.bbg_wire_encode, form, src, n, np.zeros((n, wb), dtype=np.uint8), (int(check),), strict)

    def wire_decode_device(self, form, d_wire, n, d_native, d_status=None, d_bad=None):
        """Device pointers (16-byte aligned data, n uint32 status words or None, one uint32 count or None); asynchronous on the context
        stream (bbg_wire_decode_device)."""
        self._ck(self.lib.bbg_wire_decode_device(self.ctx, form, ctypes.c_void_p(d_wire), n, ctypes.c_void_p(d_native),
                                                 ctypes.c_void_p(d_status) if d_status else None, ctypes.c_void_p(d_bad) if d_bad else None))

    def wire_encode_device(self, form, d_native, n, check, d_wire, d_status=None, d_bad=None):
        """Device pointers as wire_decode_device; asynchronous on the context stream (bbg_wire_encode_device)."""
        self._ck(self.lib.bbg_wire_encode_device(self.ctx, form, ctypes.c_void_p(d_native), n, int(check), ctypes.c_void_p(d_wire),
                                                 ctypes.c_void_p(d_status) if d_status else None, ctypes.c_void_p(d_bad) if d_bad else None))

    # host-buffer forms (what the C++ shim binds evaluate / compute_kate_opening_coefficients / divide_by_pseudo_vanishing_polynomial to)
    def poly_evaluate(self, coeffs, z):
        a = _u64(coeffs, 4)
        zz = np.ascontiguousarray(z, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        self._ck(self.lib.bbg_poly_evaluate(self.ctx, a.ctypes.data, a.shape[0], zz.ctypes.data, out.ctypes.data))
        return out

    def kate_opening(self, src, z, in_place=False):
        """Returns (dest, F(z)); in_place=True passes dest == src the way KateCommitmentScheme::batch_open does."""
        a = _u64(src, 4).copy()
        d = a if in_place else np.empty_like(a)
        zz = np.ascontiguousarray(z, dtype=np.uint64)
        f = np.zeros(4, dtype=np.uint64)
        self._ck(self.lib.bbg_kate_opening(self.ctx, a.ctypes.data, d.ctypes.data, a.shape[0], zz.ctypes.data, f.ctypes.data))
        return d, f

    def divide_by_pseudo_vanishing(self, evals, log2_src, num_roots_cut=4):
        a = _u64(evals, 4).copy()
        log2_target = a.shape[0].bit_length() - 1
        self._ck(self.lib.bbg_divide_by_pseudo_vanishing(self.ctx, a.ctypes.data, log2_src, log2_target, num_roots_cut))
        return a

    def divide_by_pseudo_vanishing_device(self, d_evals, log2_src, log2_target, num_roots_cut=4):
        self._ck(self.lib.bbg_divide_by_pseudo_vanishing_device(self.ctx, ctypes.c_void_p(d_evals), log2_src, log2_target, num_roots_cut))

    # ---- raw device memory (for hosts without torch)
    def dev_alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._ck(self.lib.bbg_dev_alloc(self.ctx, nbytes, ctypes.byref(p)))
        return p.value

    def dev_free(self, ptr):
        self._ck(self.lib.bbg_dev_free(self.ctx, ctypes.c_void_p(ptr)))

    def dev_upload(self, ptr, array):
        a = np.ascontiguousarray(array)
        self._ck(self.lib.bbg_dev_upload(self.ctx, ctypes.c_void_p(ptr), a.ctypes.data, a.nbytes))

    def dev_download(self, ptr, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        self._ck(self.lib.bbg_dev_download(self.ctx, out.ctypes.data, ctypes.c_void_p(ptr), out.nbytes))
        return out

    def profile_enable(self, on=True):
        self._ck(self.lib.bbg_profile_enable(self.ctx, 1 if on else 0))

    def profile_get(self, name):
        """(total_ms, launches) of the named kernel since profile_enable(True)."""
        ms, cnt = ctypes.c_double(0), ctypes.c_size_t(0)
        self._ck(self.lib.bbg_profile_get(self.ctx, name.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    def field_op(self, which, op, a, b=None):
        a = _u64(a, 4)
        out = np.empty_like(a)
        bp = None
        if b is not None:
            b = _u64(b, 4)
            bp = b.ctypes.data
        self._ck(self.lib.bbg_field_op(self.ctx, which, op, a.ctypes.data, bp, out.ctypes.data, a.shape[0]))
        return out

    def limb29_op_shape(self, which, op):
        """(operand rows, result rows) of a bbg_limb29_op op; raises BbgError for an unknown (which, op).  No device work."""
        operands, results = ctypes.c_int(0), ctypes.c_int(0)
        self._ck(self.lib.bbg_limb29_op_shape(which, op, ctypes.byref(operands), ctypes.byref(results)))
        return operands.value, results.value

    def limb29_op(self, which, op, rows):
        """One primitive of the 29-bit-limb arithmetic on raw operands (bbg_limb29_op): rows is (n, operands, 9) uint32, the result
        (n, results, 9) uint32."""
        operands, results = self.limb29_op_shape(which, op)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        if rows.ndim != 3 or rows.shape[1:] != (operands, 9):
            raise ValueError(f"expected (n, {operands}, 9) uint32 rows, got {rows.shape}")
        out = np.empty((rows.shape[0], results, 9), dtype=np.uint32)
        self._ck(self.lib.bbg_limb29_op(self.ctx, which, op, rows.ctypes.data, rows.shape[0], out.ctypes.data))
        return out

    def tower_op_shape(self, op):
        """(operand rows, result rows) of a bbg_tower_op op; raises BbgError for an unknown op.  No device work."""
        operands, results = ctypes.c_int(0), ctypes.c_int(0)
        self._ck(self.lib.bbg_tower_op_shape(op, ctypes.byref(operands), ctypes.byref(results)))
        return operands.value, results.value

    def tower_op(self, op, rows):
        """One device function of the pairing arithmetic on raw operands (bbg_tower_op): rows is (n, operands, 8) uint32, the result
        (n, results, 8) uint32."""
        operands, results = self.tower_op_shape(op)
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        if rows.ndim != 3 or rows.shape[1:] != (operands, 8):
            raise ValueError(f"expected (n, {operands}, 8) uint32 rows, got {rows.shape}")
        out = np.empty((rows.shape[0], results, 8), dtype=np.uint32)
        self._ck(self.lib.bbg_tower_op(self.ctx, op, rows.ctypes.data, rows.shape[0], out.ctypes.data))
        return out

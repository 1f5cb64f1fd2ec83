"""The MSM options of bbg_set_option at their library defaults, and a context manager that sets them for a block (test tooling).

The GPU tests share one session-scoped context, so an option a test leaves at any value but its default changes every later test's
kernels.  DEFAULTS restates the initialisers in aztec-2.0_amd/csrc/bbg_internal.h (struct bbg_ctx); tests/test_msm_closed_forms_cpu.py
parses the header and fails when the two part.
"""
import contextlib

# option key -> (bbg_ctx field it sets, default value as bbg_set_option takes it)
DEFAULTS = {
    "msm_window": ("msm_window", 0),
    "msm_sort": ("msm_sort", 1),
    "msm_async_reduce": ("msm_async_reduce", 0),
    "msm_reduce_quad": ("msm_reduce_quad", 14),
    "msm_acc_waves": ("msm_acc_waves", 0),
    "msm_limbs29": ("msm_limbs29", 1),
    "msm_accumulate_quad": ("msm_accumulate_quad", 1),
    "msm_reduce_priority": ("msm_reduce_low_priority", 1),
    "msm_upload_pieces": ("msm_upload_pieces", 1),
}

# setting msm_reduce_priority synchronises the device and tears the reduce streams down (bbg_capi.hip): only set when asked for
_ON_REQUEST = ("msm_reduce_priority",)


def default(key):
    return DEFAULTS[key][1]


@contextlib.contextmanager
def msm_options(bbg, **values):
    """Sets every MSM option to `values[key]` or its library default for the block, and every one back to its default afterwards."""
    unknown = set(values) - set(DEFAULTS)
    assert not unknown, f"not an MSM option: {sorted(unknown)}"
    keys = [k for k in DEFAULTS if k not in _ON_REQUEST or k in values]
    try:
        for k in keys:
            bbg.set_option(k, values.get(k, default(k)))
        yield bbg
    finally:
        for k in keys:
            bbg.set_option(k, default(k))

"""CPU checks of the two tables that tie a context's state together (no library call): the option table of bbg_set_option
(csrc/bbg_capi.hip) against the documented keys, and the scratch list of bbg_ctx (csrc/bbg_internal.h) against the struct's members."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aztec-2.0_amd", "csrc")

OPTION_KEYS = {
    "msm_async_reduce", "msm_reduce_priority", "msm_reduce_quad", "msm_acc_waves", "msm_sort", "msm_limbs29", "msm_accumulate_quad",
    "prover_ntt_batch", "quotient_limbs29", "quotient_fuse", "msm_upload_pieces", "batch_mul_glv", "ecntt_mul", "quotient_setup_plan",
    "poly_limbs29", "prover_fused_divide", "batch_mul_lanes", "prover_msm_batch", "prover_early_cosets", "ntt_limbs29", "ntt_lds_planes",
    "msm_window", "prover_tail_window", "prover_fail_round", "ntt_tile_log", "ntt_kernel", "ntt_big_tile", "ntt_max_logr8", "ntt_max_logr",
}


def _read(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def _braced(text, head):
    """The text between the braces that follow the first match of `head`."""
    m = re.search(head, text)
    assert m, head
    start = text.index("{", m.end() - 1)
    depth = 0
    for i in range(start, len(text)):
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return text[start + 1:i]
    raise AssertionError("unbalanced braces after " + head)


def test_option_table_holds_exactly_the_documented_keys():
    table = _braced(_read(CSRC, "bbg_capi.hip"), r"const Option OPTIONS\[\]\s*=\s*\{")
    keys = re.findall(r'^\s*\{\s*"([a-z0-9_]+)"', table, re.M)
    assert len(OPTION_KEYS) == 29
    assert len(keys) == len(set(keys)), sorted(k for k in keys if keys.count(k) > 1)
    assert set(keys) == OPTION_KEYS, (sorted(set(keys) - OPTION_KEYS), sorted(OPTION_KEYS - set(keys)))
    header = _read(ROOT, "include", "bbg.h")
    for key in keys:
        assert f'"{key}"' in header, f"{key} is an option of bbg_set_option that include/bbg.h does not mention"


def test_scratch_list_names_every_buffer_of_the_context():
    text = _read(CSRC, "bbg_internal.h")
    members = set(re.findall(r"^\s*(?:bbg::)?DevBuf\s+(\w+)\s*;", _braced(text, r"struct bbg_ctx\s*\{"), re.M))
    assert {"msm", "msm_tiny", "staging"} <= members, members
    listed = re.findall(r"&bbg_ctx::(\w+)", _braced(text, r"BBG_CTX_SCRATCH\[\]\s*=\s*\{"))
    assert len(listed) == len(set(listed)), listed
    assert set(listed) == members - {"msm", "msm_tiny"}, (sorted(members - set(listed)), sorted(set(listed) - members))

"""Lagrange-base SRS transform (bbg_srs_lagrange): what can be checked without a GPU.

The fixture tests/golden/lagrange_srs.json holds the output of the reference's own lagrange_base::transform_srs on the hashed synthetic
SRS.  Here it is checked against an independent model built only from the C oracle (tests/tools/lagrange_model.py), which pins the index
order and the n^-1 factor; the GPU tests reuse that model."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import lagrange_model as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANGLED = "_ZN12barretenberg13lagrange_base13transform_srsEPNS_14group_elements14affine_elementINS_5fieldINS_13Bn254FqParamsEEENS3_INS_13Bn254FrParamsEEENS_13Bn254G1ParamsEEESA_m"


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "lagrange_srs.json")) as f:
        return json.load(f)


def fixture_points(fixture, lg):
    return np.frombuffer(bytes.fromhex(fixture["points"][str(lg)]), dtype=np.uint64).reshape(-1, 8)


@pytest.mark.parametrize("lg", [1, 2, 3, 4, 5, 6])
def test_fixture_matches_the_oracle_model(fixture, oracle, lg):
    """LB[k] = msm_naive([n^-1 w^(-jk)]_j, M) equals the point the reference recorded, canonically, for every k."""
    n = 1 << lg
    assert fixture["srs"] == "hashed"
    pts = oracle.srs_hashed(fixture["srs_seed"], n)
    want = fixture_points(fixture, lg)
    assert want.shape == (n, 8)
    assert np.array_equal(lm.canon_points(oracle, want), want), "the fixture's points are not canonical"
    for k in range(n):
        assert oracle.g1_on_curve(want[k])
        assert np.array_equal(lm.lagrange_point(oracle, pts, lg, k), want[k]), f"2^{lg}: LB[{k}] differs from the model"


def test_fixture_digest_sizes(fixture):
    assert sorted(fixture["sha256"]) == ["10", "12", "8"]
    assert all(re.fullmatch(r"[0-9a-f]{64}", v) for v in fixture["sha256"].values())
    assert sorted(int(k) for k in fixture["points"]) == [1, 2, 3, 4, 5, 6]


def test_group_law_edge_family_closed_form(oracle):
    """M_j = P for j < n-1, M_{n-1} = R: LB[0] = n^-1 ((n-1) P + R) and LB[k] = n^-1 w^k (R - P) for k != 0 -- the closed form the GPU
    edge-case test uses at n = 1024, confirmed here against the model at n = 4 and 64."""
    G = oracle.g1_generator()
    P = oracle.g1_mul(G, lm.ints_to_mont(oracle, [0x1F2E3D4C5B6A7988])[0])
    R = oracle.g1_mul(G, lm.ints_to_mont(oracle, [0x0123456789ABCDEF1])[0])
    for lg in (2, 6):
        n = 1 << lg
        pts = np.stack([P] * (n - 1) + [R])
        want = edge_family_expected(oracle, P, R, lg, range(n))
        for k in range(n):
            assert np.array_equal(lm.lagrange_point(oracle, pts, lg, k), want[k]), (lg, k)


def edge_family_expected(oracle, P, R, lg, ks):
    n = 1 << lg
    w, n_inv = lm.root(oracle, lg), pow(n, lm.R_MOD - 2, lm.R_MOD)
    neg_one = lm.ints_to_mont(oracle, [lm.R_MOD - 1])[0]
    diff = oracle.g1_add(R, oracle.g1_mul(P, neg_one))  # R - P
    out = []
    for k in ks:
        if k == 0:
            s = oracle.g1_add(oracle.g1_mul(P, lm.ints_to_mont(oracle, [n - 1])[0]), R)
            out.append(oracle.g1_mul(s, lm.ints_to_mont(oracle, [n_inv])[0]))
        else:
            out.append(oracle.g1_mul(diff, lm.ints_to_mont(oracle, [n_inv * pow(w, k, lm.R_MOD)])[0]))
    return lm.canon_points(oracle, np.stack(out))


def test_entry_point_declared_bound_and_wrapped(pkg):
    header = open(os.path.join(ROOT, "include", "bbg.h")).read()
    assert re.search(r"int\s+bbg_srs_lagrange\(bbg_ctx\* ctx, bbg_srs\* srs, unsigned log2n, bbg_srs\*\* out\);", header)
    assert "bbg_srs_lagrange" in pkg.binding.EXPORTED_SYMBOLS
    assert callable(getattr(pkg.binding.Srs, "lagrange"))
    flags = []
    for name in sorted(os.listdir(os.path.join(ROOT, "shim"))):
        if re.fullmatch(r"wrap_flags.*\.txt", name):
            flags += open(os.path.join(ROOT, "shim", name)).read().split()
    assert "-Wl,--wrap=" + MANGLED in flags
    demangled = subprocess.run(["c++filt", MANGLED], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
    aff = "barretenberg::group_elements::affine_element<barretenberg::field<barretenberg::Bn254FqParams>, barretenberg::field<barretenberg::Bn254FrParams>, barretenberg::Bn254G1Params>"
    assert demangled == f"barretenberg::lagrange_base::transform_srs({aff}*, {aff}*, unsigned long)"
    shim = open(os.path.join(ROOT, "shim", "bbg_barretenberg_shim.cpp")).read()
    assert MANGLED in shim and "bbg_srs_lagrange" in shim

"""CPU tests (no GPU) for the kd-tree beam caster's selector (mcl3dl_hip_set_beam_raycast) and for the oracle the GPU
tests of tests/test_gpu_beam_kdtree.py compare against."""
import os
import re

import numpy as np
import pytest

import beam_kdtree_cases as cases
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [k for k in ("port", "ref") if pyoracle.available(k)]
NEW_SYMBOLS = ("mcl3dl_hip_set_beam_raycast", "mcl3dl_hip_get_beam_raycast", "mcl3dl_hip_group_set_beam_raycast")


def test_selector_is_declared_and_bound():
    from mcl_3dl_amd import capi
    header = open(os.path.join(ROOT, "include", "mcl3dl_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = capi.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in capi.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.mcl3dl_hip_abi_version() == 3
    for cls in (capi.Engine, capi.Group):
        assert callable(getattr(cls, "set_beam_raycast")) and callable(getattr(cls, "get_beam_raycast"))
    # a null context is refused before anything is touched
    assert lib.mcl3dl_hip_set_beam_raycast(None, 1) == -1
    assert lib.mcl3dl_hip_get_beam_raycast(None, None) == -1
    assert lib.mcl3dl_hip_group_set_beam_raycast(None, 1) == -1


@pytest.mark.skipif(len(KINDS) < 2, reason="oracle/_ref not built here (needs /root/reference at build time)")
@pytest.mark.parametrize("case", sorted(cases.STATUS_CASES, key=str), ids=str)
def test_ref_and_port_agree_on_the_kdtree_caster(case):
    dist_weight, flm = case
    ref = cases.oracle_statuses("ref", dist_weight, flm, False)
    port = cases.oracle_statuses("port", dist_weight, flm, False)
    np.testing.assert_array_equal(ref[0], port[0])
    np.testing.assert_array_equal(ref[1], port[1])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", sorted(cases.STATUS_CASES, key=str), ids=str)
def test_oracle_meets_the_coverage_conditions(kind, case):
    """What keeps the GPU comparison from passing vacuously: all four statuses occur, in the recorded numbers, and the
    kd-tree caster's answer differs from the DDA caster's in at least 400 of the 2000 rays."""
    dist_weight, flm = case
    st, hit = cases.oracle_statuses(kind, dist_weight, flm, False)
    counts = tuple(int(np.sum(st == s)) for s in range(4))
    assert counts == cases.STATUS_CASES[case]
    assert min(counts) > 0
    assert np.all((hit >= 0) == (st != 2))
    st_dda, _ = cases.oracle_statuses(kind, dist_weight, flm, True)
    assert not np.any(st_dda == 3)  # RaycastUsingDDA reports sin_angle = 1: never TOTAL_REFLECTION
    assert int(np.sum(st != st_dda)) >= 400

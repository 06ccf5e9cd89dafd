"""The weight-gradient rules of the engines' backward passes on the CPU: ctta_wgrad_plan (the plan the U-Net's and the VAE
decoder's backward launch from) against decisions RECORDED from the two selection routines as they were before they became
one plan.

tests/golden/wgrad_plan_cases.json: one line per case, [name, policy, geometry, plan] -- `policy`: "unet" or "vae"
(ctta_wgrad_engine_policy 0 / 1), `geometry`: the ctta_wgrad_geom fields in their declared order, `plan`: the
ctta_wgrad_plan_info fields in their declared order.  The table was made before the split: the selection expressions of the
U-Net's wgrad_slabs and of the VAE's vconv_wgrad -- route conditions, split loops, mp / seg / R / ld, sums_apart, the direct
conditions, the buffer sizes -- were copied unchanged into a stand-alone host program linked against the library (for
ctta_wgrad_implicit_supported), which printed one line per case: the layers the comments and profiles name, and a sample of
the grid C, N in {8 .. 1280} x widths {1 .. 128} x heights {1 .. 1024} x B in {1, 2, 9} x taps {1, 9} x (async, dY kept
alive) x direct permitted, filled up until every route, the split caps and S == 1 are met often enough.  The VAE's routine
admits stride-1 layers without per-sample columns on the caller's stream, so its cases are those.  A rule that changes what
some layer launches, or what scratch it takes, changes one of these."""
import ctypes
import json
import os

import pytest

import abi
from consistencytta_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOM = [f for f, _ in N.WgradGeom._fields_]
PLAN = [f for f, _ in N.WgradPlanInfo._fields_]
ROUTES = ("tn", "tn_direct", "implicit_inplace", "implicit_direct", "implicit_dyt", "im2col_t")
ENGINE = {"unet": 0, "vae": 1}
REACHES = {"unet": set(ROUTES), "vae": {"tn", "implicit_inplace", "im2col_t"}}

with open(os.path.join(ROOT, "tests", "golden", "wgrad_plan_cases.json")) as _f:
    CASES = [dict(name=n, policy=p, geom=dict(zip(GEOM, g)), plan=dict(zip(PLAN, r))) for n, p, g, r in json.load(_f)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def policy(lib, name):
    p = N.WgradPolicy()
    assert lib.ctta_wgrad_engine_policy(ENGINE[name], ctypes.byref(p)) == 0
    return p


def test_case_table_is_what_the_issue_asks_for(lib):
    assert len(CASES) >= 400 and len({c["name"] for c in CASES}) == len(CASES)
    assert all(len(c["geom"]) == len(GEOM) and len(c["plan"]) == len(PLAN) for c in CASES)
    for pol, routes in REACHES.items():
        cap = policy(lib, pol).implicit_cap
        mine = [c["plan"] for c in CASES if c["policy"] == pol]
        for r in routes:
            assert sum(1 for p in mine if ROUTES[p["route"]] == r) >= 10, (pol, r)
        assert not [p for p in mine if ROUTES[p["route"]] not in routes]
        assert sum(1 for p in mine if ROUTES[p["route"]].startswith("implicit") and p["splits"] == cap) >= 20, pol
    assert sum(1 for c in CASES if c["plan"]["splits"] == 1) >= 20


def test_the_two_policies(lib):
    u, v = policy(lib, "unet"), policy(lib, "vae")
    assert (u.implicit_target, u.implicit_cap, u.direct, u.upsample_copy) == (256, 16, 1, 0)
    assert (v.implicit_target, v.implicit_cap, v.direct, v.upsample_copy) == (512, 128, 0, 1)
    assert lib.ctta_wgrad_engine_policy(2, ctypes.byref(u)) != 0


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_equals_recorded_decision(lib, case):
    out = N.WgradPlanInfo()
    st = lib.ctta_wgrad_plan(ctypes.byref(N.WgradGeom(**case["geom"])), ctypes.byref(policy(lib, case["policy"])), ctypes.byref(out))
    assert st == 0, lib.ctta_last_error().decode()
    diff = {f: (getattr(out, f), case["plan"][f]) for f in PLAN if getattr(out, f) != case["plan"][f]}
    assert not diff, "field: (planned, recorded) %r" % diff


def test_header_signatures_and_library_agree_on_the_new_entries(lib):
    abi.assert_bound(("ctta_wgrad_plan", "ctta_wgrad_engine_policy"), lib)

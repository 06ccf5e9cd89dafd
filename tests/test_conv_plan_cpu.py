"""conv_gemm's dispatch rules on the CPU: ctta_conv_plan (the plan ctta_conv_gemm launches from) against plans RECORDED
from the dispatcher as it was before it was split into plan and launch steps.

tests/golden/conv_plan_cases.json: one line per case, [name, desc, env, status, plan or error text] -- `desc`: the
ctta_conv_desc fields that differ from expand_desc()'s defaults (pointer fields are 1 = bound / 0 = NULL and never
dereferenced), `env`: the ctta_conv_plan_env fields that differ from ENV0, and what the recorder saw: `status` and the
ctta_conv_plan_info fields in their declared order, trailing zeros dropped (kernel, grids, split / tail / tile-order /
stream-K schedule, epilogue flags, profiler code) or the ctta_last_error() text.  A rule that changes what some shape
launches changes one of these."""
import ctypes
import json
import os

import pytest

from consistencytta_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
PTRS = ("x0", "x1", "w", "bias", "bias_m", "rowvec", "res", "out", "out2", "gn_part")
FIELDS = [f for f, _ in N.ConvPlanInfo._fields_]
HDR = 8192          # ctta_conv_workspace_header_bytes()
ENV0 = dict(cu_count=256, xcd=1, splitk=1, streamk=1, streamk_grid=0, suppress_splitk=0, stamps_bound=0,
            workspace_bytes=192 << 20, workspace_header_zeroed=1)



def expand_desc(d):
    """The full descriptor of a case: a 1x1 stride-1 problem on one pixel per sample with x0 / w / out bound, output extent
    = input extent, ldc = n and k_pad = K rounded up to 64, unless the case says otherwise."""
    f = dict(x0=1, w=1, out=1, hi=1, wi=1, kh=1, kw=1, stride_h=1, stride_w=1, dil_h=1, dil_w=1, alpha=1.0)
    f.update(d)
    f.setdefault("ho", f["hi"])
    f.setdefault("wo", f["wi"])
    f.setdefault("ldc", f.get("n", 0))
    f.setdefault("k_pad", (f["kh"] * f["kw"] * (f.get("c0", 0) + (f.get("c1", 0) if f.get("x1") else 0)) + 63) // 64 * 64)
    return f


def _load():
    with open(os.path.join(HERE, "golden", "conv_plan_cases.json")) as f:
        rows = json.load(f)
    return [dict(name=n, desc=expand_desc(d), env=dict(ENV0, **e), status=st, **({"error": r} if st else {"plan": dict(zip(FIELDS, r + [0] * len(FIELDS)))}))
            for n, d, e, st, r in rows]


CASES = _load()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        N.build()
    return N.lib()


def make_desc(fields):
    d = N.ConvDesc()
    for k, v in fields.items():
        setattr(d, k, (0x1000 if v else None) if k in PTRS else v)
    return d


def plan(lib, desc, env):
    """(status, plan dict or error text)"""
    out = N.ConvPlanInfo()
    st = lib.ctta_conv_plan(ctypes.byref(make_desc(desc)), ctypes.byref(N.ConvPlanEnv(**env)), ctypes.byref(out))
    if st:
        return st, lib.ctta_last_error().decode()
    return st, {f: getattr(out, f) for f in FIELDS}


def linear(M, n, K, **kw):
    return expand_desc(dict(c0=K, batch=M, n=n, **kw))


def test_case_table_is_what_the_issue_asks_for():
    assert len(CASES) >= 300 and len({c["name"] for c in CASES}) == len(CASES)
    assert sum(1 for c in CASES if c["status"]) >= 25
    assert all(set(c["plan"]) == set(FIELDS) for c in CASES if not c["status"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_equals_recorded_plan(lib, case):
    st, got = plan(lib, case["desc"], case["env"])
    assert st == case["status"], got
    if st:
        assert got == case["error"]
    else:
        diff = {f: (got[f], case["plan"][f]) for f in FIELDS if got[f] != case["plan"][f]}
        assert not diff, "field: (planned, recorded) %r" % diff


def test_undersized_streamk_workspace_is_an_error(lib):
    # a workspace smaller than its own stream-K header (plus two partial-tile slots): the clamp of the grid to the
    # workspace used to underflow here and the launch wrote out of bounds
    for ws in (1, 4096, HDR - 1, HDR, HDR + 256 * 256 * 4, HDR + 2 * 256 * 256 * 4):
        for desc in (linear(4608, 1024, 9216), linear(2048, 1024, 4096, tile=41)):
            st, err = plan(lib, desc, dict(ENV0, workspace_bytes=ws))
            assert st == 1 and err == "conv_gemm: workspace too small for stream-K", (ws, st, err)
    st, got = plan(lib, linear(4608, 1024, 9216), dict(ENV0, workspace_bytes=HDR + 2 * 256 * 256 * 4 + 1))
    assert st == 0 and (got["variant"], got["grid_x"]) == (41, 1)


def _factor(tiles, nk):
    return max(1, min(512 // tiles, 8, nk // 8))


def _auto_tile22_shape(tiles):
    """(M, N) with `tiles` 64x128 tiles that the rules send to tile 22 at K >= 4096 (deep and narrow, M <= 640, N >= 256) --
    and not to the big tile's deep case (N % 256 == 0 with 64 or more 256x256 tiles)"""
    for a in range(1, 11):
        b = tiles // a
        if tiles % a == 0 and b >= 2 and (b % 2 == 1 or -(-a * 64 // 256) * (b // 2) < 64):
            return 64 * a, 128 * b
    return None


def test_ring_rule_and_schedule_use_one_splitk_factor(lib):
    """tiles 1..191 x nk 32..512 of the 64x128x64 tile.  The schedule's factor shows in every plan (forced tile 22: K tiles
    per split = ceil(nk / factor)); the ring rule's shows where the rules reach tile 22 by themselves (K >= 4096): it moves
    the launch to the 3-stage ring (27) exactly when factor * tiles lies in (384, 512] (M <= 640: thin_ring) or fills
    whole rounds of 512 slots to 85 %."""
    ring_seen = set()
    for tiles in range(1, 192):
        auto = _auto_tile22_shape(tiles)
        for nk in range(32, 513):
            f = _factor(tiles, nk)
            nk_split = -(-nk // f)
            splits = -(-nk // nk_split)
            want = (splits, nk_split if splits > 1 else nk)
            st, got = plan(lib, linear(64, 128 * tiles, 64 * nk, tile=22), ENV0)
            assert st == 0 and (got["variant"], got["splits"], got["nk_split"]) == (22,) + want, (tiles, nk, got)
            if auto and nk >= 64:
                wgs = tiles * f
                ring = (wgs >= 512 and wgs * 100 >= -(-wgs // 512) * 512 * 85) or 384 < wgs <= 512
                st, got = plan(lib, linear(auto[0], auto[1], 64 * nk), ENV0)
                assert st == 0 and (got["variant"], got["splits"], got["nk_split"]) == (27 if ring else 22,) + want, (tiles, nk, got)
                ring_seen.add(ring)
    assert ring_seen == {True, False}

"""The cases of tests/brox_cases.py are what their names say -- halo layout, tile width, K, last-tile interior, deep plan,
k_coarse split -- so that no GPU test of tests/test_brox_limits_gpu.py can move off its branch unnoticed; the restated
pyramid is the oracle's; and a pyramid level of one pixel is refused by the oracle and by hm_brox_create alike, before
anything runs."""
import ctypes
import os
import subprocess
import sys

import pytest

import brox_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", [c["name"] for c in bc.CASES])
def test_case_is_on_its_branch(name):
    c = bc.CASES_BY_NAME[name]
    d = bc.derived(c)
    for k, v in c["expect"].items():
        assert d[k] == v, (name, k, d[k], v)
    for q in bc.plan(c):
        if q is not None:
            # the halo of a tiled axis is 2K, and the interior of every tile -- the last one included -- is not empty
            assert q["step_x"] > 0 and q["step_y"] > 0
            assert q["last_x"] is None or 1 <= q["last_x"] <= q["step_x"]
            assert q["last_y"] is None or 1 <= q["last_y"] <= q["step_y"]


def test_the_table_covers_every_branch():
    seen = set()
    for c in bc.CASES:
        for q in bc.plan(c):
            if q is None:
                continue
            seen.add(("layout", q["layout"], q["tw"]))
            seen.add(("deep", q["deep"]))
            for last in (q["last_x"], q["last_y"]):
                if last in (1, 2):
                    seen.add(("last", q["K"], last))
        seen.add(("coarse", any(q is None for q in bc.plan(c))))
    want = {("layout", lay, tw) for lay in ("fit_both", "fit_x", "fit_y", "tiled") for tw in (64, 128)}
    want |= {("deep", True), ("deep", False), ("coarse", True), ("coarse", False)}
    want |= {("last", K, last) for K in (5, 10) for last in (1, 2)}
    assert want <= seen, want - seen
    knobs = [c["knobs"] for c in bc.CASES]
    assert {0, 8} <= {k.get("sor_deep", 1) for k in knobs} and {0, 10} <= {k.get("sor_fuse", 0) for k in knobs}
    params = [bc.oracle_kw(c) for c in bc.CASES]
    for key, vals in (("alpha", (0.1, 0.4)), ("gamma", (25.0, 100.0)), ("inner", (5, 20)), ("solver", (5, 12, 13, 20)),
                      ("scale", (0.5, 0.2, 0.1, 0.99)), ("outer", (1, 2))):
        assert set(vals) <= {p[key] for p in params}, key


def test_wide_tile_changes_the_plan():
    """three pairs of 336 x 336, sor_deep 1, 256 CUs: K = 10 on the wide tile (4 x 14 x 3 = 168 tiles of 1024 threads
    fit 256 x 1024 slots), K = 5 on the narrow one (14 x 14 x 3 = 588 tiles of 512 threads do not)"""
    c = bc.CASES_BY_NAME["wide_deep:336x336"]
    wide, narrow = bc.plan(c)[0], bc.plan(c, sor_wide=0)[0]
    assert (wide["tw"], wide["K"], wide["tiles_x"], wide["tiles_y"]) == (128, 10, 4, 14)
    assert (narrow["tw"], narrow["K"], narrow["threads"]) == (64, 5, 512)
    # two pairs never take the wide tile
    assert bc.plan(dict(c, n=2))[0]["tw"] == 64


def test_deep_plan_boundary():
    assert bc.sor_plan(100, 100, 12, slots=256)["K"] == 12
    assert bc.sor_plan(100, 100, 12, slots=256)["step_x"] == 16
    assert bc.sor_plan(100, 100, 13, slots=256)["K"] == 1
    assert bc.sor_plan(100, 100, 10, slots=0)["K"] == 5              # sor_deep 0
    assert bc.sor_plan(100, 100, 20, fuse=10, slots=256)["halo_x"] == 20


def test_coarse_split_at_the_level_cap():
    lv = bc.levels(64, 64, 0.99, 200)
    assert len(lv) == bc.MAX_LEVELS
    kc, launches = bc.coarse_split(lv, 64)
    assert kc == 0 and [hi - lo + 1 for _, lo, hi in launches] == [32, 27, 32, 32, 5]
    assert [T for T, _, _ in launches] == [32, 32, 64, 64, 64]
    kc, launches = bc.coarse_split(lv, 32)
    assert all(w > 32 or h > 32 for w, h in lv[:kc]) and [T for T, _, _ in launches] == [32, 32]
    assert bc.coarse_split(lv, 0) == (len(lv), [])


@pytest.mark.parametrize("name", [c["name"] for c in bc.CASES])
def test_levels_are_the_oracles(oracle_brox, name):
    c = bc.CASES_BY_NAME[name]
    p = bc.oracle_kw(c)
    assert oracle_brox.levels(c["W"], c["H"], p["scale"], p["outer"]) == bc.levels(c["W"], c["H"], p["scale"], p["outer"])
    assert bc.one_pixel_level(c["W"], c["H"], p["scale"], p["outer"]) is None


def test_second_level_of_the_narrow_strips(oracle_brox):
    assert oracle_brox.levels(16, 200)[1] == (13, 160)
    assert oracle_brox.levels(200, 16)[1] == (160, 13)


def test_oracle_refuses_one_pixel_levels(oracle_brox):
    """a 1 x 1 frame (all-NaN flow before) and 64 x 64 at scale 0.01 (levels 64^2, 1^2: the oracle crashed in bilin on
    the NaN flow): ValueError, and the process that asked goes on"""
    assert [bc.one_pixel_level(W, H, s) for W, H, s in bc.REFUSED] == [0, 1]
    script = (
        "import numpy as np\n"
        "from oracle import brox_oracle as o\n"
        "for W, H, s in %r:\n"
        "    f = np.full((H, W), 0.5, np.float32)\n"
        "    try:\n"
        "        o.calc(f, f, scale=s)\n"
        "    except ValueError:\n"
        "        print('refused', W, H, s)\n"
        "f = np.zeros((2, 2), np.float32)\n"
        "u, v = o.calc(f, f)\n"
        "print('alive', bool(np.isfinite(u).all() and np.isfinite(v).all()))\n" % (bc.REFUSED,))
    r = subprocess.run([sys.executable, "-c", script], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:3] == ["refused 1 1 0.8", "refused 64 64 0.01", "alive True"], r.stdout


def test_hm_brox_create_refuses_one_pixel_levels_without_a_gpu(hm):
    """refused before the device is touched: the same answer on a machine without a GPU"""
    from hydra_mi import _lib
    L = _lib.lib()
    h = _lib.c_vp()
    for (W, H, s), level in zip(bc.REFUSED, (0, 1)):
        assert L.hm_brox_create(0, W, H, 1, 0.197, 50.0, s, 10, 77, 10, ctypes.byref(h)) == -1
        msg = L.hm_last_error().decode()
        assert "level %d is 1x1" % level in msg and "%dx%d" % (W, H) in msg and "%g" % s in msg, msg
        assert not h.value

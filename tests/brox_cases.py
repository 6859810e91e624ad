"""Frames, parameters and tuning knobs shared by the CPU and GPU tests of the Brox flow at its structural limits
(csrc/brox.hip: make_levels, sor_plan / k_sor, the k_coarse split; csrc/brox_kernels.h: the mirrored-border stencils).

Each limit changes a code path, and every case here sits on one side of one of them:
  sor_plan's halo layouts: a level fits the SOR tile on x (w <= tile width, 64 or 128 for the wide tile), on y
      (h <= 64), on both (all `solver` iterations in one launch, no halo) or on neither (halo 2K on either axis);
  the last tile of a row or column with an interior of 1 or 2 px (w or h = 1, 2 mod step) at K = 5 (step 44) and
      K = 10 (step 24);
  the deep plan: all `solver` iterations in one launch when step = TW - 4 solver >= 16, solver <= 15 and the tiles
      fit sor_deep x CUs workgroup slots (solver 12 is deep with step 16, 13 is not and, prime, runs K = 1);
  the wide tile (k_sor<128, 64, 1024>), only for calls of more than two pairs;
  the k_coarse split: the levels of at most coarse_max px a side, COARSE_MAX = 32 levels per launch and one launch per
      tile size, up to the 128-level cap of the pyramid;
  the mirrored borders of images narrower than a stencil: the 5-tap derivatives at w < 3, the blur at w < R
      (R = 2, 4, 9 and the clamp 16 at scale 0.8, 0.5, 0.2, 0.1).

Every case is a dict: name, W, H, n (pairs per call), params (brox_oracle.calc's names), knobs (hm_brox_tune) and
expect: what the restated plan of level `level` must be -- the branch the case is about.  The host restatement of
sor_plan and of the k_coarse split below predicts the SOR launches of every level (inner x solver / K), which is all
that hm_brox_profile_levels counts."""
import zlib

import numpy as np

SOR_TW = 64                 # tile width (the wide tile: twice that) and height of k_sor
SOR_TH = 64
COARSE_MAX = 32             # levels per k_coarse launch
MAX_LEVELS = 128
MI355X_CUS = 256
DEFAULTS = dict(alpha=0.197, gamma=50.0, scale=0.8, inner=10, outer=77, solver=10)
KNOBS = dict(sor_threads=0, sor_fuse=0, sor_deep=1, sor_wide=0, coarse_max=32)
FIELDS = ("warp", "rotate", "translate_leftup", "translate_leftup_stretch")


def levels(W, H, scale=0.8, outer=77):
    """make_levels: ceil(W s^k) x ceil(H s^k) with s^k accumulated in binary32, while the last level exceeds 15 px on
    both sides, fewer than `outer` levels and fewer than 128"""
    out = [(int(W), int(H))]
    sc = np.float32(1.0)
    s = np.float32(scale)
    while out[-1][0] > 15 and out[-1][1] > 15 and len(out) < outer and len(out) < MAX_LEVELS:
        sc = np.float32(sc * s)
        w = max(1, int(np.ceil(np.float32(W) * sc)))
        h = max(1, int(np.ceil(np.float32(H) * sc)))
        out.append((w, h))
    return out


def one_pixel_level(W, H, scale=0.8, outer=77):
    """index of the first 1 x 1 level (refused by hm_brox_create and the oracle), or None"""
    for k, (w, h) in enumerate(levels(W, H, scale, outer)):
        if w == 1 and h == 1:
            return k
    return None


def sor_plan(w, h, solver, fuse=0, threads=1024, n=1, slots=0, wide=0):
    """sor_plan of csrc/brox.hip, term for term"""
    tw = 2 * SOR_TW if (wide > 0 and w >= wide and h >= wide) else SOR_TW
    if tw != SOR_TW:
        threads = 1024
    fitx, fity = w <= tw, h <= SOR_TH
    deep = False
    if fuse > 0:
        K = fuse
    elif fitx and fity:
        K = solver
    else:
        K = max(d for d in range(1, min(5, solver) + 1) if solver % d == 0)
        step = tw - 4 * solver
        if step >= 16 and solver <= 15:
            tiles = (1 if fitx else -(-w // step)) * (1 if fity else -(-h // (SOR_TH - 4 * solver))) * n
            if tiles * threads <= slots * 1024:
                K, deep = solver, True
    halo_x = 0 if fitx else 2 * K
    halo_y = 0 if fity else 2 * K
    step_x, step_y = tw - 2 * halo_x, SOR_TH - 2 * halo_y
    tiles_x = 1 if fitx else -(-w // step_x)
    tiles_y = 1 if fity else -(-h // step_y)
    layout = {(True, True): "fit_both", (True, False): "fit_x", (False, True): "fit_y", (False, False): "tiled"}
    return dict(K=K, threads=threads, tw=tw, deep=deep, layout=layout[fitx, fity], halo_x=halo_x, halo_y=halo_y,
                step_x=step_x, step_y=step_y, tiles_x=tiles_x, tiles_y=tiles_y,
                last_x=w - (tiles_x - 1) * step_x if not fitx else None,        # interior of the last tile
                last_y=h - (tiles_y - 1) * step_y if not fity else None)


def coarse_split(lv, coarse_max):
    """(kc, launches): levels kc.. run inside k_coarse, as launches (T, lo, hi) from the coarsest level up -- one per
    tile size T and at most COARSE_MAX levels each"""
    L = len(lv)
    kc = L
    while kc > 0 and lv[kc - 1][0] <= coarse_max and lv[kc - 1][1] <= coarse_max:
        kc -= 1
    tile = lambda g: 32 if g[0] <= 32 and g[1] <= 32 else 64
    out, hi = [], L - 1
    while hi >= kc:
        T, lo = tile(lv[hi]), hi
        while lo - 1 >= kc and hi - (lo - 1) + 1 <= COARSE_MAX and tile(lv[lo - 1]) == T:
            lo -= 1
        out.append((T, lo, hi))
        hi = lo - 1
    return kc, out


def plan(c, cus=MI355X_CUS, **over):
    """per level of case c (knobs overridden by `over`): None inside k_coarse, else the restated sor_plan with
    'launches' = the SOR launches of one call"""
    p = dict(DEFAULTS, **c["params"])
    k = dict(KNOBS, **c["knobs"])
    k.update(over)
    n = c["n"]
    lv = levels(c["W"], c["H"], p["scale"], p["outer"])
    kc, _ = coarse_split(lv, k["coarse_max"])
    threads = k["sor_threads"] or (1024 if n <= 2 else 512)
    out = []
    for i, (w, h) in enumerate(lv):
        if i >= kc:
            out.append(None)
            continue
        q = sor_plan(w, h, p["solver"], k["sor_fuse"], threads, n, k["sor_deep"] * cus, k["sor_wide"] if n > 2 else 0)
        q["launches"] = p["inner"] * (p["solver"] // q["K"])
        out.append(q)
    return out


def launches(c, cus=MI355X_CUS, **over):
    """SOR launches per level of one call (0 for the levels inside k_coarse)"""
    return [0 if q is None else q["launches"] for q in plan(c, cus, **over)]


def case(name, W, H, n=1, params=None, knobs=None, level=0, expect=None, sweep=False):
    return dict(name=name, W=W, H=H, n=n, params=dict(params or {}), knobs=dict(knobs or {}), level=level,
                expect=dict(expect or {}), sweep=sweep)


WIDE = dict(sor_wide=64)

CASES = [
    # the four halo layouts of the 64 x 64 tile (one pair: 1024 threads)
    case("fit_x:1x300", 1, 300, expect=dict(layout="fit_x", tw=64), sweep=True),
    case("fit_x:2x200", 2, 200, expect=dict(layout="fit_x", tw=64)),
    case("fit_x:33x129", 33, 129, expect=dict(layout="fit_x", tw=64), sweep=True),
    case("fit_x:64x65", 64, 65, expect=dict(layout="fit_x", tw=64), sweep=True),
    case("fit_y:300x1", 300, 1, expect=dict(layout="fit_y", tw=64)),
    case("fit_y:129x33", 129, 33, expect=dict(layout="fit_y", tw=64), sweep=True),
    case("fit_both:64x64", 64, 64, expect=dict(layout="fit_both", tw=64, K=10)),
    case("tiled:131x97", 131, 97, expect=dict(layout="tiled", tw=64)),
    # ... and of the wide tile (three pairs: the wide tile is only used for calls of more than two)
    case("wide_fit_x:100x300", 100, 300, n=3, knobs=WIDE, expect=dict(layout="fit_x", tw=128, threads=1024), sweep=True),
    case("wide_fit_y:300x64", 300, 64, n=3, knobs=WIDE, expect=dict(layout="fit_y", tw=128, threads=1024)),
    case("wide_fit_both:128x64", 128, 64, n=3, knobs=WIDE, expect=dict(layout="fit_both", tw=128, K=10)),
    # the wide tile where it changes the plan: K = 10 (wide, 4 x 14 tiles x 3 pairs fit the chip) against K = 5 (narrow)
    case("wide_deep:336x336", 336, 336, n=3, params=dict(outer=4), knobs=WIDE,
         expect=dict(layout="tiled", tw=128, K=10, deep=True)),
    case("narrow_not_deep:336x336", 336, 336, n=3, params=dict(outer=4),
         expect=dict(layout="tiled", tw=64, K=5, deep=False)),
    # last tiles with an interior of 1 / 2 px: K = 5 (sor_deep 0: step 44) and K = 10 (deep: step 24)
    case("last_1x_2y:K5:89x90", 89, 90, knobs=dict(sor_deep=0), expect=dict(K=5, step_x=44, last_x=1, last_y=2)),
    case("last_2x_1y:K5:90x133", 90, 133, knobs=dict(sor_deep=0), expect=dict(K=5, step_x=44, last_x=2, last_y=1)),
    case("last_1x_2y:K10:73x74", 73, 74, expect=dict(K=10, deep=True, step_x=24, last_x=1, last_y=2)),
    case("last_2x_1y:K10:98x97", 98, 97, expect=dict(K=10, deep=True, step_x=24, last_x=2, last_y=1)),
    # the deep plan on and off
    case("deep:solver12", 100, 100, params=dict(solver=12), expect=dict(K=12, deep=True, step_x=16)),
    case("not_deep:solver13", 100, 100, params=dict(solver=13), expect=dict(K=1, deep=False)),
    case("deep_off:sor_deep0", 100, 100, knobs=dict(sor_deep=0), expect=dict(K=5, deep=False)),
    case("deep:sor_deep8:336x336", 336, 336, n=3, params=dict(outer=3), knobs=dict(sor_deep=8),
         expect=dict(layout="tiled", tw=64, threads=512, K=10, deep=True)),
    # solver 20: four passes of 5, or two of 10 with a 20 px halo
    case("solver20:fuse0", 100, 100, params=dict(solver=20), expect=dict(K=5, deep=False, launches=40)),
    case("solver20:fuse10", 100, 100, params=dict(solver=20), knobs=dict(sor_fuse=10),
         expect=dict(K=10, halo_x=20, step_x=24, launches=20)),
    # small frames: single levels, mirrored stencils wider than the image
    case("small:1x2", 1, 2, expect=dict(coarse=True)),
    case("small:2x1", 2, 1, expect=dict(coarse=True)),
    case("small:2x2", 2, 2, expect=dict(coarse=True)),
    case("small:3x5", 3, 5, expect=dict(coarse=True)),
    case("small:5x3", 5, 3, expect=dict(coarse=True)),
    case("small:5x5", 5, 5, expect=dict(coarse=True)),
    case("small:15x15", 15, 15, expect=dict(coarse=True)),
    case("small:16x16", 16, 16, expect=dict(coarse=True)),
    case("small:16x200", 16, 200, expect=dict(layout="fit_x")),
    case("small:200x16", 200, 16, expect=dict(layout="fit_y")),
    case("small:40x300", 40, 300, expect=dict(layout="fit_x")),
    # the reference's parameter study (scripts/opticflowtests.sh): one value off the defaults at a time
    case("alpha0.1", 120, 90, params=dict(alpha=0.1)),
    case("alpha0.4", 120, 90, params=dict(alpha=0.4)),
    case("gamma25", 120, 90, params=dict(gamma=25.0)),
    case("gamma100", 120, 90, params=dict(gamma=100.0)),
    case("inner5", 120, 90, params=dict(inner=5), expect=dict(K=10, launches=5)),
    case("inner20", 120, 90, params=dict(inner=20), expect=dict(K=10, launches=20)),
    case("solver5", 120, 90, params=dict(solver=5), expect=dict(K=5, deep=True)),
    case("solver20", 120, 90, params=dict(solver=20), expect=dict(K=5, launches=40)),
    # blur radii 4, 9 and the clamp 16: levels narrower than the blur (5 x 4 at 0.2) and lower than the derivative (3 x 2 at 0.1)
    case("scale0.5", 150, 100, params=dict(scale=0.5)),
    case("scale0.2", 100, 80, params=dict(scale=0.2), level=2, expect=dict(w=5, h=4, coarse=True)),
    case("scale0.1", 200, 160, params=dict(scale=0.1), level=2, expect=dict(w=3, h=2, coarse=True)),
    case("outer1", 120, 90, params=dict(outer=1), expect=dict(nlevels=1)),
    case("outer2", 120, 90, params=dict(outer=2), expect=dict(nlevels=2)),
    # the 128-level cap: five k_coarse launches at coarse_max 64 (32 + 32 + 5 levels of the 64 tile, 32 + 27 of the 32)
    case("levels128:scale0.99", 64, 64, params=dict(scale=0.99, outer=200), knobs=dict(coarse_max=64),
         expect=dict(nlevels=128, coarse_launches=5, coarse=True)),
]

CASES_BY_NAME = {c["name"]: c for c in CASES}
REFUSED = [(1, 1, 0.8), (64, 64, 0.01)]          # W, H, scale: a 1 x 1 level (level 0; level 1)


def derived(c, cus=MI355X_CUS, **over):
    """what `expect` may name, at the case's level"""
    p = dict(DEFAULTS, **c["params"])
    k = dict(KNOBS, **c["knobs"])
    k.update(over)
    lv = levels(c["W"], c["H"], p["scale"], p["outer"])
    q = plan(c, cus, **over)[c["level"]]
    d = dict(q or {})
    d.update(coarse=q is None, nlevels=len(lv), w=lv[c["level"]][0], h=lv[c["level"]][1],
             coarse_launches=len(coarse_split(lv, k["coarse_max"])[1]))
    return d


def frames(c, seed=0):
    """n pairs of u8 frames (n, H, W): crops of the synthetic warps, one field per pair"""
    from hydra_mi import synth
    N = max(c["W"], c["H"], 8)
    N += N & 1
    s0 = zlib.crc32(c["name"].encode()) % 1000 + seed
    F0, F1 = [], []
    for i in range(c["n"]):
        f0, f1, _, _ = synth.warp_pair(N, FIELDS[i % 4], s0 + i)
        F0.append(np.ascontiguousarray(f0[:c["H"], :c["W"]]))
        F1.append(np.ascontiguousarray(f1[:c["H"], :c["W"]]))
    return np.stack(F0), np.stack(F1)


def oracle_kw(c):
    return dict(DEFAULTS, **c["params"])


def create_kw(c):
    """BroxOpticalFlow's names for the case's parameters"""
    p = oracle_kw(c)
    return dict(alpha=p["alpha"], gamma=p["gamma"], scale_factor=p["scale"], inner_iterations=p["inner"],
                outer_iterations=p["outer"], solver_iterations=p["solver"])

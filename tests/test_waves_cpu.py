"""Activity waves without a GPU: the rule of hm_body_rec_waves as tests/waves_ref.py restates it, on inputs whose answers
are known by hand, and the host side of hydra_mi.waves (velocity, triggers, origin, the command's refusals).  Every
comparison is an equality."""
import os
import sys

import numpy as np
import pytest

import waves_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = ref.NONE


def _waves():
    sys.path.insert(0, ROOT)
    from hydra_mi import waves
    return waves


def _one(trace, t, pre, lead, post, min_rise):
    """a single map pixel with the trace as its plane -> (lat, rise, why)"""
    y = np.asarray(trace, np.uint8).reshape(-1, 1, 1)
    m = np.ones((1, 1), bool)
    lat, rise, why = ref.event(*ref.binned(y, m, 0), m, t, pre, lead, post, min_rise)
    return int(lat[0, 0]), int(rise[0, 0]), int(why[0, 0])


def _plane_wave(F=40, n=24, t=10):
    """baseline 0, a ramp 0, 50, 100, 150, 200 that starts at the trigger and comes half a frame later per column"""
    k, x = np.arange(F)[:, None, None], np.arange(n)[None, None, :]
    return np.broadcast_to(np.clip(50 * (k - t) - 25 * x, 0, 200), (F, n, n)).astype(np.uint8)


def test_planted_plane_wave_latency_gradient_and_velocity():
    w = _waves()
    t, n = 10, 24
    y, m = _plane_wave(t=t), np.ones((n, n), bool)
    assert list(y[t:t + 6, 0, 0]) == [0, 50, 100, 150, 200, 200] and list(y[t:t + 7, 0, 2]) == [0, 0, 50, 100, 150, 200, 200]
    o = ref.waves(y, m, [t], 0, 4, 2, 20, 8, 4, 3)
    assert (o["why"] == 0).all() and (o["n_bin"] == 1).all() and (o["rise"] == 4 * 200).all()
    x = np.arange(n)
    # half height (100) is reached at frame t + 2 + x / 2: on a frame for even columns (k_x = that frame, frac = 256)
    assert np.array_equal(o["lat"][0], np.broadcast_to(256 * 2 + 128 * x, (n, n)))
    kx = t + 2 + x[::2] // 2
    assert np.array_equal(o["lat"][0][:, ::2], np.broadcast_to(256 * (kx - t), (n, n // 2)))
    g, v = w.velocity(o["fit"], 49)
    gr, vr = ref.velocity(o["fit"], 49)
    assert np.array_equal(g, gr, equal_nan=True) and np.array_equal(v, vr, equal_nan=True)
    g, v = g[0].reshape(6, 6, 2), v[0].reshape(6, 6, 2)                  # nodes at 0, 4, .., 20: windows inside from 4 to 20
    assert (g[1:, 1:] == (0.5, 0.0)).all() and (v[1:, 1:] == (2.0, 0.0)).all()
    assert np.isnan(g[0]).all() and np.isnan(g[:, 0]).all()              # fewer than 49 pixels at the border
    cnt = o["cnt"]
    mean, sd = w.mean_sd(cnt, o["sum_lat"], o["sum_lat2"])
    assert np.array_equal(mean, np.broadcast_to(2 + x / 2, (n, n)).astype(np.float32)) and not sd.any()
    assert w.origin(mean, cnt, 1) == (0, 0)
    nodes = np.stack(np.meshgrid(np.arange(0, n, 4), np.arange(0, n, 4)), -1).reshape(-1, 2)
    gm, vm = w.mean_velocity(mean, cnt, nodes, 3, 1, n_min=49)
    assert (gm.reshape(6, 6, 2)[1:, 1:] == (0.5, 0.0)).all() and (vm.reshape(6, 6, 2)[1:, 1:] == (2.0, 0.0)).all()
    # the wave the other way and along the rows
    o = ref.waves(np.ascontiguousarray(y[:, :, ::-1].transpose(0, 2, 1)), m, [t], 0, 4, 2, 20, 8, 4, 3)
    g, v = w.velocity(o["fit"], 49)
    assert (g[0].reshape(6, 6, 2)[1:, 1:] == (0.0, -0.5)).all() and (v[0].reshape(6, 6, 2)[1:, 1:] == (0.0, -2.0)).all()


def test_codes_ties_and_plateaus():
    #       frame 0  1  2  3  4   5   6    7    8    9   10
    rise = [0, 0, 0, 0, 0, 40, 80, 80, 60, 80, 10]
    # two frames attain the maximum 80: k_M is the first (6), so the window's end at 9 is no "still rising"
    assert _one(rise, 4, 2, 0, 5, 8) == (256 * (5 - 1 - 4) + 256, 160, 0)
    assert _one(rise, 4, 2, 0, 2, 8) == (256, 160, 1)                       # the window ends at frame 6, the first maximum
    # a plateau at half height: the first frame that reaches it counts
    assert _one([0, 0, 0, 50, 50, 50, 100, 0], 2, 2, 0, 5, 8) == (256 * (3 - 1 - 2) + 256, 200, 0)
    # a plateau just below it: the crossing is in the step that follows
    assert _one([0, 0, 0, 49, 49, 100, 0], 2, 2, 0, 4, 8) == (256 * (5 - 1 - 2) + (256 * (200 - 4 * 49)) // (4 * 51), 200, 0)
    # code 3: at half height when the search starts (baseline 10, 10; maximum 90; theta = 20 + 180; 4 x 50 >= 200)
    assert _one([10, 10, 50, 90, 0], 2, 2, 0, 2, 8) == (NONE, 160, 3)
    assert _one([10, 10, 49, 90, 0], 2, 2, 0, 2, 8) == (256 * (3 - 1 - 2) + (256 * (200 - 4 * 49)) // (4 * 41), 160, 0)     # one below: a crossing
    assert _one([10, 10, 49, 90, 0], 2, 2, 0, 1, 8)[2] == 1                  # ... and with the window's end at the maximum, still rising
    # code 2: a rise one below pre n min_rise = 3 x 1 x 8 = 24, and exactly at it
    assert _one([5, 5, 5, 5, 12, 12, 0], 3, 3, 0, 2, 8) == (NONE, 21, 2)
    assert _one([5, 5, 6, 5, 13, 13, 0], 3, 3, 0, 2, 8) == (NONE, 3 * 13 - 16, 2)
    assert _one([5, 5, 5, 5, 13, 13, 0], 3, 3, 0, 2, 8)[1:] == (24, 0)
    assert _one([9, 9, 9, 3, 3, 3], 3, 3, 0, 2, 1) == (NONE, -18, 2)          # a fall: R < 0, no crossing
    # lead: the baseline ends `lead` frames before the trigger, and the latency may be negative
    assert _one([0, 0, 0, 100, 100, 100, 100], 4, 2, 2, 2, 8) == (256 * (3 - 1 - 4) + 128, 200, 0)
    # still rising at the window's end
    assert _one([0, 0, 10, 20, 30, 40, 50, 60], 2, 2, 0, 3, 8) == (256 * (3 - 1 - 2) + 256, 80, 1)      # frames 2..5: maximum 40 at the end, 20 at frame 3


def test_bins_over_the_maps_edge():
    m = np.zeros((9, 10), bool)
    m[2:7, 1:8] = True
    m[2, 1] = m[6, 7] = False                                               # two corners cut: no rectangle
    rng = np.random.default_rng(3)
    y = rng.integers(0, 256, (12, 9, 10)).astype(np.uint8)
    for b in (0, 1, 2, 8):
        Y, n = ref.binned(y, m, b)
        for r in range(9):
            for c in range(10):
                rr, cc = slice(max(r - b, 0), r + b + 1), slice(max(c - b, 0), c + b + 1)
                assert n[r, c] == m[rr, cc].sum() and Y[5, r, c] == int(y[5][rr, cc][m[rr, cc]].sum())
    o = ref.waves(y, m, [6], 1, 2, 1, 3, 8, 2, 2)
    assert o["n_bin"][4, 4] == 9 and o["n_bin"][2, 2] == 5 and o["n_bin"][3, 1] == 5 and o["n_bin"][2, 1] == 0 and o["n_bin"][0, 0] == 0
    assert (o["why"][0][~m] == 255).all() and (o["lat"][0][~m] == NONE).all() and not o["rise"][0][~m].any()
    assert (o["why"][0][m] != 255).all() and o["n_bin"][m].min() >= 1
    assert ref.nodes(m, 2) == (4, 3, 1, 2) and ref.nodes(m, 64) == (1, 1, 1, 2) and o["fit"].shape == (1, 12, 9)
    valid = o["why"][0] <= 1
    assert o["fit"][0, :, 0].max() <= 25 and o["fit"][0, 0, 0] == valid[0:5, 0:4].sum()      # node (1, 2): columns -1..3, rows 0..4
    # an empty map: the box is one pixel, off the map
    o = ref.waves(y, np.zeros((9, 10), bool), [6], 1, 2, 1, 3, 8, 2, 2)
    assert (o["why"] == 255).all() and not o["cnt"].any() and not o["fit"].any() and not o["n_bin"].any()


def test_triggers_refractory_and_both_ends():
    w = _waves()
    ev = np.zeros(60, bool)
    ev[[3, 4, 5, 12, 20, 21, 30, 55]] = True
    assert list(w.onsets(ev, 1)) == [3, 12, 20, 30, 55]                      # the first frame of every run
    assert list(w.onsets(ev, 9)) == [3, 12, 30, 55]                          # 20 is 8 after 12; 30 is 18 after 12
    assert list(w.onsets(ev, 10)) == [3, 20, 30, 55]                         # 12 is 9 after 3: dropped, so 20 counts from 3
    assert list(w.admissible([3, 4, 5, 55, 56, 57], 2, 2, 3, 60)) == [False, True, True, True, True, False]
    F = 120
    y = np.zeros((2, F))
    for k in (3, 40, 44, 80, 117):                                           # sharp events that decay with g = 0.5
        y[0, k:] += 100.0 * 0.5 ** np.arange(F - k)
    y[1] = y[0][::-1]                                                       # a trace that only falls into its events
    t = w.triggers(y, g=0.5, lam=0.0, s_min=50.0, refractory=8, pre=2, lead=2, post=3, F=F)
    assert len(t) == 2 and t[0].dtype == np.int32 and list(t[0]) == [40, 80]   # 3 and 117: windows off the ends; 44: refractory
    assert list(w.triggers(y[0], g=0.5, lam=0.0, s_min=50.0, refractory=4, pre=2, lead=1, post=2, F=F)[0]) == [3, 40, 44, 80, 117]
    assert list(w.triggers(y[0], g=0.5, lam=0.0, s_min=50.0, refractory=4, pre=2, lead=1, post=2, F=119)[0]) == [3, 40, 44, 80]
    auto = w.triggers(y[0] + np.random.default_rng(0).normal(0, 1, F), pre=2, lead=2, post=3)[0]
    assert set([40, 80]) <= set(auto.tolist())
    assert w.triggers(np.full((1, 20), np.nan))[0].size == 0


def test_origin_ties_and_velocity_nans():
    w = _waves()
    lm = np.array([[3.0, 1.0, 1.0], [1.0, 0.5, np.nan]], np.float32)
    cnt = np.array([[5, 2, 3], [3, 1, 0]], np.uint32)
    assert w.origin(lm, cnt, 1) == (1, 1) and w.origin(lm, cnt, 2) == (1, 0) and w.origin(lm, cnt, 3) == (2, 0)
    assert w.origin(lm, cnt, 6) is None and w.origin(lm, cnt, 0) == (1, 1)
    # the sums of three pixels (0, 0), (1, 0), (0, 1) with Lat 0, 256, 512: g = (1, 2) frames per pixel
    f = np.array([[3, 1, 1, 1, 0, 1, 768, 256, 512]], np.int64)
    g, v = w.velocity(f, 3)
    assert g.tolist() == [[1.0, 2.0]] and v.tolist() == [[1.0 / 5.0, 2.0 / 5.0]]
    assert np.isnan(w.velocity(f, 4)[0]).all() and np.isnan(w.velocity(f, 4)[1]).all()          # n < n_min
    line = np.array([[3, 3, 0, 5, 0, 0, 768, 1280, 0]], np.int64)           # (0, 0), (1, 0), (2, 0): a singular A
    assert np.isnan(w.velocity(line, 1)[0]).all()
    flat = np.array([[3, 1, 1, 1, 0, 1, 300, 100, 100]], np.int64)          # the same latency everywhere: no direction
    assert np.isnan(w.velocity(flat, 1)[1]).all()
    assert np.isnan(w.velocity(np.zeros((2, 4, 9), np.int64), 0)[0]).all()
    for fit in (f, line, flat):
        for a, b in zip(w.velocity(fit, 1), ref.velocity(fit, 1)):
            assert np.array_equal(a, b, equal_nan=True)
    with pytest.raises(ValueError):
        w.velocity(f.astype(np.int32), 1)


def test_colour_map(tmp_path):
    w = _waves()
    lm = np.full((4, 5), np.nan)
    lm[1, 1], lm[1, 2], lm[2, 2] = 1.0, 2.0, 3.0
    gray = np.full((4, 5), 100, np.uint8)
    out = w.colour_map(lm, gray, str(tmp_path / "m.png"))
    assert out.shape == (4, 5, 3) and (out[0] == 100).all()
    assert out[1, 1].tolist() == [(100 + 255 + 1) >> 1, (100 + 0 + 1) >> 1, (100 + 0 + 1) >> 1]          # the earliest: blue
    assert out[2, 2].tolist() == [(100 + 0 + 1) >> 1, (100 + 0 + 1) >> 1, (100 + 255 + 1) >> 1]          # the latest: red
    assert os.path.getsize(str(tmp_path / "m.png")) > 0
    assert (w.colour_map(np.full((4, 5), np.nan), gray) == 100).all()


REFUSALS = [
    (["--waves-pre", "4"], "--waves-pre goes with --waves"),
    (["--waves-map", "m.png"], "--waves-map goes with --waves"),
    (["--waves-keep"], "--waves-keep goes with --waves"),
    (["--waves-frames", "t.txt"], "--waves-frames goes with --waves"),
    (["--waves", "--waves-frames", "t.txt"], "--waves works on the kept record: it needs --rois or --demix"),
    (["--points", "p.csv", "--rois", "--waves"], "--waves needs trigger frames: the ensembles of --network or a file of them (--waves-frames)"),
    (["--points", "p.csv", "--rois", "--network", "--waves", "--waves-bin", "9"], "--waves-bin 9 outside 0..8"),
    (["--points", "p.csv", "--rois", "--network", "--waves", "--waves-pre", "0"], "--waves-pre 0 outside 1..64"),
    (["--points", "p.csv", "--rois", "--waves", "--waves-frames", "t.txt", "--waves-post", "257"], "--waves-post 257 outside 1..256"),
    (["--points", "p.csv", "--rois", "--waves", "--waves-frames", "t.txt", "--waves-fit", "17"], "--waves-fit 17 outside 1..16"),
    (["--points", "p.csv", "--rois", "--network", "--waves", "--dff-gain", "0"], "the running baseline needs a --detrend-half in 0..1024"),
    (["--points", "p.csv", "--rois", "--waves", "--waves-frames", "t.txt"], "--waves-frames t.txt cannot be read: No such file or directory"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: " ".join(c[0]))
def test_the_command_refuses_before_anything_touches_a_gpu(case, monkeypatch, tmp_path, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("COLUMNS", "200")
    sys.path.insert(0, ROOT)
    import run_kalmanfilter as cli
    with pytest.raises(SystemExit) as exc:
        cli.main(["nofile.npy", "noflow", "out.npz"] + case[0])          # (names that do not exist: nothing is opened)
    assert exc.value.code == 2
    err = " ".join(capsys.readouterr().err.split())
    assert "error: " in err and case[1] in err
    assert os.listdir(".") == []


def test_the_file_of_trigger_frames_is_read_before_anything_is_tracked(monkeypatch, tmp_path, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("COLUMNS", "200")
    sys.path.insert(0, ROOT)
    import run_kalmanfilter as cli
    argv = ["nofile.npy", "noflow", "out.npz", "--points", "p.csv", "--rois", "--waves", "--waves-frames", "t.txt"]
    (tmp_path / "t.txt").write_text("12 30\n4.5\n")
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2 and "--waves-frames t.txt holds something that is no whole number" in " ".join(capsys.readouterr().err.split())
    (tmp_path / "t.txt").write_text("12 30\n 41\n\n")
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    cli.check_args(parser, args)
    assert args.waves_trigger_frames.tolist() == [12, 30, 41] and args.waves_trigger_frames.dtype == np.int64
    assert cli.read_trigger_frames(str(tmp_path / "t.txt")).tolist() == [12, 30, 41]


def test_without_waves_the_options_stay_unset_and_the_stage_does_nothing():
    sys.path.insert(0, ROOT)
    import run_kalmanfilter as cli
    parser = cli.build_parser()
    args = parser.parse_args(["a.npy", "flow", "out.npz"])
    cli.check_args(parser, args)
    assert not args.waves and args.waves_pre == 8 and args.waves_post == 24 and args.waves_bin == 2
    assert cli.stage_waves(None, args) is None                            # (it looks at nothing of the run)
    assert cli.STAGES.index(cli.stage_network) < cli.STAGES.index(cli.stage_waves) < cli.STAGES.index(cli.stage_record_end)

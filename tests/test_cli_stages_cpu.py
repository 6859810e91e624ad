"""CPU checks of run_kalmanfilter.py as a whole: every refusal of the command line with its words (and, where two
apply, which one wins), and the order of its stages -- with every library call stubbed by a recorder, the list of calls,
the names in the states file in their order and the printed lines are compared with what the command did before its
main() was cut into stages.  No GPU, no native library."""
import contextlib
import io
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, H, W, T = 4, 8, 8, 1                      # frames of the stub video (F - 1 states), its size, triangles
S = F - 1
IO = ["nofile.npy", "noflow", "out.npz"]     # names that do not exist: no refusal below opens a file


def _cli():
    sys.path.insert(0, ROOT)
    import run_kalmanfilter as cli
    return cli


# ---- every refusal --------------------------------------------------------------------------------------------------------
PTS, ROIS = ["--points", "p.csv"], ["--points", "p.csv", "--rois"]
FIND = ["--find-points", "5"]
REFUSALS = [            # (argv after the three names, words of the message[, words of a later refusal that must not show])
    (["--depth-range", "5"], "--depth-range takes two whole numbers A,B, not '5'"),
    (["--depth-range", "1,2", "--depth-percentiles", "1,2"], "not both"),
    (["--depth-gamma", "0"], "--depth-gamma takes a positive number"),
    (["--video-quality", "0"], "--video-quality is 1..100"),
    (["--strain-alpha", "256"], "the strain video needs a --strain-alpha in 0..255 and a finite --strain-gain"),
    (["--strain-gain", "inf"], "the strain video needs a --strain-alpha in 0..255 and a finite --strain-gain"),
    (["--cells-video", "c.avi"], "--cells-video draws cells or points: it needs one of --points, --find-points, --rois, --demix"),
    (["--cells-video-states", "filtered"], "--cells-video-states goes with --cells-video"),
    (PTS + ["--cells-video", "c.avi", "--cells-video-states", "smoothed"], "--cells-video-states smoothed needs --smooth"),
    (FIND + PTS, "--find-points finds the points itself: not together with --points"),
    (["--find-points", "0"], "--find-points needs N >= 1 and a --find-radius in 1..16"),
    (FIND + ["--find-radius", "17"], "--find-points needs N >= 1 and a --find-radius in 1..16"),
    (["--points-out", "o.csv"], "--points-out goes with --find-points"),
    (["--find-min-score", "0.5"], "--find-min-score is the least score of --find-points: it needs --find-points and a finite number"),
    (FIND + ["--find-min-score", "nan"], "--find-min-score is the least score of --find-points"),
    (FIND + ["--find-more", "2"], "--find-more looks beside the points found: it needs --find-points and --find-min-score"),
    (FIND + ["--find-min-score", "0.1", "--find-more", "0"], "--find-more needs at least one round and a --find-blank >= 0"),
    (PTS + ["--residual-video", "r.avi"], "--residual-video shows what the demixed model leaves: it needs --demix or --find-more"),
    (PTS + ["--demix", "--demix-iters", "0"], "--demix-iters needs at least one round"),
    (["--rois"], "--rois reads cells out: it needs --find-points or --points"),
    (["--demix"], "--rois reads cells out: it needs --find-points or --points"),
    (["--events"], "--events reads the cells' traces: it needs --rois or --demix"),
    (["--events-video", "e.avi"], "--events-video shows the events: it needs --events"),
    (ROIS + ["--events", "--events-g", "1.0"], "--events-g must lie inside 0 < g < 1"),
    (ROIS + ["--events", "--events-lambda=-1"], "--events-lambda and --events-smin must be finite and >= 0"),
    (ROIS + ["--events", "--events-smin", "nan"], "--events-lambda and --events-smin must be finite and >= 0"),
    (["--network"], "--network reads the cells' traces: it needs --rois or --demix"),
    (["--network-map", "m.png"], "--network-map draws the ensembles: it needs --network"),
    (ROIS + ["--network", "--network-lag=-1"], "--network needs a --network-lag >= 0 and finite thresholds"),
    (ROIS + ["--network", "--network-thr", "nan"], "--network needs a --network-lag >= 0 and finite thresholds"),
    (["--network-null", "5"], "--network-null tests the ensembles' maps: it needs --network"),
    (["--network-guard=-1"], "--network-null and --network-guard must be >= 0 and --network-alpha in (0, 1]"),
    (["--network-alpha", "0"], "--network-null and --network-guard must be >= 0 and --network-alpha in (0, 1]"),
    (["--detrend"], "--detrend finds the cells in the excess video: it needs --find-points"),
    (["--resummarize"], "--resummarize sums the stabilised record up: it needs --stabilize, and not --detrend"),
    (["--dff-video", "d.avi", "--detrend-half", "2000"], "the running baseline needs a --detrend-half in 0..1024, a --detrend-q in "
     "0..100, a --dff-floor in 1..255 and a --dff-gain in 1..65535"),
    (ROIS + ["--events", "--dff-gain", "0"], "the running baseline needs a --detrend-half in 0..1024"),
    (["--stabilize"], "--stabilize works on the kept record: it needs --rois or --demix"),
    (ROIS + ["--stabilize", "--stab-patch", "3"], "--stabilize needs a --stab-patch in 4..64, a --stab-search in 0..8 and at least one pass"),
    (["--deform-correct"], "--deform-correct works on the kept record: it needs --rois or --demix"),
    (["--deform-gamma", "1.0"], "--deform-gamma needs --deform-correct and an exponent in 0..3"),
    (ROIS + ["--deform-correct", "--deform-gamma", "4"], "--deform-gamma needs --deform-correct and an exponent in 0..3"),
    (["--pca", "2"], "--pca reads the kept record: it needs --rois or --demix"),
    (ROIS + ["--pca", "0"], "--pca needs at least one component"),
    (["--pca-frames"], "--pca-frames adds the frame similarity: it needs --pca"),
    (["--deep-traces"], "--deep-traces reads cells out of the 16-bit frames: it needs --rois, --demix or --points"),
    (ROIS + ["--deep-traces", "--stabilize"], "--deep-traces reads the frames as they were tracked: --stabilize rewrites the kept "
     "record, and the second pass does not repeat that"),
    (ROIS + ["--deep-traces", "--deform-correct"], "--deep-traces reads the frames as they were tracked: --deform-correct rewrites "
     "the kept record, and the second pass does not repeat that"),
    (PTS + ["--deep-traces", "--deep-offset", "nan"], "--deep-offset needs a finite number"),
    (["--deep-offset", "3"], "--deep-offset goes with --deep-traces"),
    # two refusals apply: the first in the command's order of checks is the one the user reads
    (FIND + PTS + ["--find-radius", "17"], "not together with --points", "--find-radius in 1..16"),
    (["--events", "--network"], "--events reads the cells' traces", "--network reads"),
    (["--stabilize", "--deform-correct"], "--stabilize works on the kept record", "--deform-correct works"),
]


def _refused(cli, argv, words, capsys, loser=None):
    before = sorted(os.listdir("."))
    with pytest.raises(SystemExit) as exc:
        cli.main(argv)
    assert exc.value.code == 2
    err = " ".join(capsys.readouterr().err.split())               # (argparse wraps the message to the terminal)
    assert "error: " in err and words in err
    if loser is not None:
        assert loser not in err
    assert sorted(os.listdir(".")) == before and not os.path.exists(argv[2])


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: " ".join(c[0]))
def test_refusal_that_needs_no_file(case, monkeypatch, tmp_path, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("COLUMNS", "200")
    _refused(_cli(), IO + case[0], case[1], capsys, *case[2:])


def test_the_table_covers_every_refusal_site():
    """one case at least per parser.error of the command line: 43 sites, four of them below (they need the input)"""
    import inspect
    import re
    src = inspect.getsource(_cli())
    sites = re.findall(r"parser\.error\(\s*\"((?:[^\"\\]|\\.)*)\"", src)
    assert len(sites) >= 42                                       # (43 sites when this was written; one passes depth_of's message on)
    table = [c[1] for c in REFUSALS] + ["--deep-traces reads 16-bit frames: ", "-t/--threshold ",
                                          "--pca: a record of ", "--pca: "]
    for text in sites:                                            # (the message's first literal, up to what is filled in)
        head = text.split("%")[0]
        assert any(head in words for words in table), text


@pytest.fixture
def tiny(monkeypatch, tmp_path):
    """a 6 x 32 x 32 video with a bright square, 8-bit and 16-bit; the host path of the 16-bit mapping"""
    rng = np.random.default_rng(0)
    v = rng.integers(0, 8, (6, 32, 32)).astype(np.uint8)
    v[:, 8:24, 8:24] += 100
    np.save(str(tmp_path / "v8.npy"), v)
    np.save(str(tmp_path / "v16.npy"), v.astype(np.uint16) * 16)
    cli = _cli()
    monkeypatch.setattr(cli.deepio, "default_device", lambda: None)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("COLUMNS", "200")
    return cli


def test_refusals_that_need_the_input(tiny, monkeypatch, capsys):
    cli = tiny
    _refused(cli, ["v8.npy", "noflow", "out.npz"] + PTS + ["--deep-traces"],
             "--deep-traces reads 16-bit frames: v8.npy holds none (8-bit input has no more depth than the kept record)", capsys)
    _refused(cli, ["v16.npy", "noflow", "out.npz", "-t", "300"],
             "-t/--threshold 300: with 16-bit input the threshold lies in 0..255, the scale of the mapped frames", capsys)
    _refused(cli, ["v8.npy", "noflow", "out.npz"] + ROIS + ["--pca", "9"], "--pca: 9 components of 5 frames (need 1..4)", capsys)
    monkeypatch.setattr(cli.pca, "GRAM_MAX", 3)
    _refused(cli, ["v8.npy", "noflow", "out.npz"] + ROIS + ["--pca", "2"],
             "--pca: a record of 5 frames, one Gram matrix takes 3 at the most", capsys)


# ---- the order of the stages, with stubs ----------------------------------------------------------------------------------
class _Log(list):
    def fn(self, name, ret=None):
        """a recorder: notes its name (and whether it was handed video options), returns `ret` or ret(*args)"""
        def call(*a, **kw):
            self.append(name + (" +video_opts" if "video_opts" in kw else ""))
            return ret(*a, **kw) if callable(ret) else ret
        return call

    def obj(self, prefix, methods, **attrs):
        o = types.SimpleNamespace(**attrs)
        for name, ret in methods.items():
            setattr(o, name, self.fn(prefix + "." + name, ret))
        return o

    def patch(self, monkeypatch, module, prefix, methods):
        for name, ret in methods.items():
            monkeypatch.setattr(module, name, self.fn(prefix + name, ret))


def _z(*shape, dtype=np.float64):
    return np.zeros(shape, dtype)


def _cells(n):
    """what roi.extract and demix.extract give for n cells"""
    labels = np.full((H, W), -1, np.int32)
    labels[0, :n] = np.arange(n)
    return dict(shapes=_z(n, 17, 17), shapes_q=_z(n, 17, 17, dtype=np.uint8), C=_z(S, n), dff_demixed=_z(S, n),
                demix_change=np.array([0.5, 0.25]), footprints=_z(n, 17, 17), roi_labels=labels, roi_counts=np.full(n, 9),
                ring_counts=np.full(n, 20), F_roi=_z(S, n), F_np=_z(S, n), dff=_z(S, n), seed_fallback=_z(n, dtype=bool))


def _read(kf_or_body, states, *a):
    pts = a[-2]
    return dict(points=_z(len(states), len(pts), 2), point_means=_z(len(states), len(pts)), point_counts=_z(len(pts)))


FOUND = np.array([[2.5, 3.5], [5.5, 4.5]])


def _stub(monkeypatch, flow_files=False, record=64, deep=False):
    """run_kalmanfilter with every name it calls replaced by a recorder -> (module, the list of calls)"""
    cli, log = _cli(), _Log()
    img = lambda: dict(mean=_z(H, W), std=_z(H, W), max=_z(H, W), corr=_z(H, W), frames=S)

    class Video:
        def __init__(self, src, threshold):
            log.append("VideoStream(%s)" % (src if isinstance(src, str) else "mapped frames"))
            self.frames, self.frame, self.k = _z(F, H, W, dtype=np.uint8), _z(H, W, dtype=np.uint8), 0

        current_frame = lambda self: self.frame
        backsub = lambda self: (self.frame, None, None)
        isOpened = lambda self: self.k < F

        def read(self):
            self.k += 1
            return self.k < F, self.frame, self.frame, self.frame

    class Writer:
        def __init__(self, path, W, H, **opts):                    # (raw: no codec keyword at all)
            log.append("AviWriter(%s%s)" % (path, "".join(", %s=%r" % kv for kv in sorted(opts.items()))))
            self.frames, self.write = S, log.fn("%s.write" % path)
            self.close = log.fn("%s.close" % path)

    class Smoother:
        def __init__(self, kf, frames, covariances, max_bytes):
            log.append("RTSSmoother(%d)" % frames)
            self.n, self.run, self.close = 0, log.fn("sm.run", (_z(S, 8), np.ones((S, 8)))), log.fn("sm.close")

        def record(self):
            self.n += 1

        __len__ = lambda self: self.n

    class Stack(cli.deepio.TiffStack):                             # (a TIFF stack is what the command closes itself)
        def __init__(self, name):
            self.close = log.fn(name + ".close")

    def kf(distmesh, frame, flow, cuda, **kw):
        log.append("IteratedMSKalmanFilter(cuda=%r)" % cuda)
        renderer = log.obj("renderer", dict(body_map=(_z(H, W, dtype=np.int32),), body_stats_end=None, body_rec_end=None,
                                            view=_z(H, W, 3, dtype=np.uint8)))
        state = types.SimpleNamespace(X=_z(8, 1), tri=_z(T, 3, dtype=np.int32), renderer=renderer)
        return log.obj("kf", dict(compute=(0, 0.0, 0.0, 0, None, None), screenshots=None), state=state, N=2)

    def body(kf, points=None, point_radius=3.0, video=None, stats=False, keep=False, keep_bytes=0):
        log.append("BodyReadout(stats=%r, keep=%r)" % (stats, keep))
        L = 0 if points is None else len(points)
        res = dict(tri_means=_z(S, T), tri_counts=_z(T), points=_z(S, L, 2), point_means=_z(S, L), point_counts=_z(L))
        return log.obj("body", dict(results=res, summary=img(), find_points=(FOUND, np.array([0.9, 0.8])), frame=None,
                                    locate=lambda pts: (_z(len(pts), dtype=np.int32),)),
                       outside=np.array([False, True][:L]), keep=keep, L=L, labels=_z(H, W, dtype=np.int32), label_counts=np.ones(L))

    def pipeline(kf, source):
        log.append("FlowEKFPipeline(%s)" % type(source).__name__)

        def run(on_frame, video, body, smoother):
            for k in range(S):
                on_frame(k, (0, 0.0, 0.0, 0))
                if smoother is not None:
                    smoother.record()
        return log.obj("pipe", dict(run=run, close=None))

    for name, stub in dict(VideoStream=Video, AviWriter=Writer, RTSSmoother=Smoother, BodyReadout=body,
                           FlowEKFPipeline=pipeline).items():      # (these note themselves, with what they were given)
        monkeypatch.setattr(cli, name, stub)
    monkeypatch.setattr(cli.kalman, "IteratedMSKalmanFilter", kf)
    log.patch(monkeypatch, cli, "", dict(
        DistMesh=lambda frame, h0: log.obj("distmesh", dict(createMesh=None, size=4), p=_z(4, 2)),
        FlowStream=lambda path: types.SimpleNamespace(peek=lambda: (flow_files, _z(H, W, 2)), read=lambda: (True, _z(H, W, 2))),
        record_bytes=record, read_out=_read, read_out_recorded=_read, check_budget=None))
    more = dict(points=np.vstack((FOUND, [[6.5, 1.5]])), scores=[np.array([0.5, 0.4])], round=np.array([0, 0, 1], np.int32),
                clipped=[7], refused=[1], new_scores=np.array([0.5]), e=_cells(3))
    net = dict(r=_z(2, 2, 21), labels=np.array([0, 0, -1]), ens_traces=_z(1, S), lead_lag=_z(1, 1), lead_r=_z(1, 1),
               rho=_z(1, H, W), map=_z(H, W, dtype=np.int16), p_r=_z(2, 2), p_map=_z(1, H, W), rho_max=_z(1, 5),
               sig=_z(1, H, W, dtype=bool), map_sig=_z(H, W, dtype=np.int16), gray=_z(H, W, dtype=np.uint8))
    tri = dict(J=np.ones((S, T)), l1=np.ones((S, T)), l2=np.ones((S, T)), axis=_z(S, T), rotation=_z(S, T), body_area=np.ones(S))
    mapped = dict(frames=_z(F, H, W, dtype=np.uint8), clipped=_z(F, 2, dtype=np.int64), source=Stack("stack"), lo=100, hi=4000,
                  gamma=1.0, lo_ppm=1000, hi_ppm=999990, lut=None)            # what a 16-bit input is mapped to
    layers = lambda n: (np.tile(np.arange(n, dtype=np.int32) % max(n, 1), (2, H, W // max(n, 1) + 1))[:, :, :W], _z(2, H, W))
    for module, methods in (
            (cli.stabilize, dict(stabilize=dict(shifts=_z(S, 4, 2, dtype=np.int32), score=_z(S, 4), fallback=_z(S, 4, dtype=bool),
                                                q=_z(S, 4, 2, dtype=np.int16)))),
            (cli.deform, dict(correct=dict(gamma=0.5, fit_r2=0.75, fitted=True, gain=np.full((S, T), 4096, np.uint16), clipped=0,
                                           r_before=_z(H, W), r_after=_z(H, W)))),
            (cli.pca, dict(pca=lambda body, k, frames: dict(lam=np.ones(k), share=np.full(k, 0.25), temporal=_z(S, k),
                                                            rho=_z(k, H, W), frame_score=np.ones(S), frame_r=_z(S, S)))),
            (cli.detrend, dict(summary=img(), write_video=S)),
            (cli.residual, dict(find_more=more, write_video=(S, 0))),
            (cli.demix, dict(extract=lambda body, pts, **kw: _cells(len(pts)))),
            (cli.roi, dict(extract=lambda body, pts, **kw: _cells(len(pts)))),
            (cli.events, dict(noise=1.0, estimate_g=0.9, default_lam=0.1, default_smin=0.2, event_video=S,
                              deconvolve=lambda tr, g, lam: (np.zeros_like(tr), np.zeros_like(tr)),
                              binarise=lambda s, smin: np.zeros(s.shape, bool),
                              count_image=(_z(H, W, dtype=np.uint32), _z(H, W)))),
            (cli.network, dict(extract=net, coactivity=_z(2, 2, 21), colour_map=None, strain_coupling=_z(1, T))),
            (cli.strain, dict(triangles=tri, artifact_score=lambda J, dff: _z(J.shape[1]), write_video=S,
                              labels=lambda kf, states, **kw: {k: _z(S, kw.get("L", len(kw.get("points", ())))) for k in ("J", "l1", "l2")})),
            (cli.cellview, dict(layers_from_shapes=lambda shapes, *a: layers(len(shapes)) + (1,),
                                layers_from_labels=lambda labels: layers(int(labels.max()) + 1),
                                levels=lambda dff: _z(*dff.shape, dtype=np.uint8), write_video=S)),
            (cli.deeptrace, dict(run=_z(S, 2), columns=None, point_means=_z(S, 2),
                                 extract=lambda body, src, states, e, **kw: {k: np.ones((S, len(e["roi_counts"]))) for k in (
                                     "deep_F_roi", "deep_F_np", "deep_dff", "deep_demix_c")})),
            (cli.deepio, dict(open_deep=lambda fn: Stack("src16"), load_deep=lambda fn, depth: mapped if deep else None,
                              DeepSource=lambda *a, **kw: log.obj("DeepSource", dict(close=None))))):
        log.patch(monkeypatch, module, module.__name__.split(".")[-1] + ".", methods)
    return cli, log


def _run(monkeypatch, tmp_path, argv, **how):
    """-> (the calls in order, the names in the states file in order, the printed lines)"""
    monkeypatch.chdir(tmp_path)
    with open("p.csv", "w") as f:
        f.write("a,2.5,3.5\nb,5.5,4.5\n")
    cli, log = _stub(monkeypatch, **how)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert cli.main(argv) == 0
    fn_out = argv[2] if argv[2].endswith(".npz") else argv[2] + ".npz"
    with np.load(fn_out) as z:
        files = list(z.files)
    return list(log), files, out.getvalue().splitlines()


# name: (argv, how the stubs are set, the calls, the names in the states file, the printed lines), all three recorded from
# the command as it was before its main() was cut into stages
RUNS = {}
RUNS["everything_after_a_search"] = (
    ['in.npy', 'noflow', 'out.npz', '--find-points', '5', '--find-min-score', '0.1', '--find-more', '2', '--residual-video',
     'res.avi', '--stabilize', '--stab-mode', 'field', '--deform-correct', '--pca', '2', '--pca-frames', '--detrend',
     '--dff-video', 'dff.avi', '--events', '--events-video', 'ev.avi', '--network', '--network-null', '5', '--network-map',
     'map.png', '--strain', '--strain-video', 'strain.avi', '--cells-video', 'cells.avi', '--smooth', '--registered', 'reg.avi',
     '--points-out', 'found.csv', '--video-codec', 'mjpeg'],
    {},
    ['deepio.load_deep', 'VideoStream(in.npy)', 'DistMesh', 'distmesh.createMesh', 'distmesh.size', 'check_budget',
     'FlowStream', "AviWriter(reg.avi, channels=1, codec='mjpeg', quality=90)", 'IteratedMSKalmanFilter(cuda=True)',
     'FlowEKFPipeline(Video)', 'renderer.body_map', 'record_bytes', 'BodyReadout(stats=True, keep=True)', 'RTSSmoother(3)',
     'pipe.run', 'pipe.close', 'body.results', 'stabilize.stabilize', 'deform.correct', 'pca.pca', 'body.summary',
     'detrend.summary', 'body.find_points', 'residual.find_more', 'renderer.body_stats_end', 'read_out_recorded',
     'detrend.write_video +video_opts', 'body.locate', 'residual.write_video +video_opts', 'events.noise', 'events.noise',
     'events.noise', 'events.estimate_g', 'events.estimate_g', 'events.estimate_g', 'events.default_lam', 'events.default_lam',
     'events.default_lam', 'events.default_smin', 'events.default_smin', 'events.default_smin', 'events.deconvolve',
     'events.count_image', 'events.binarise', 'network.coactivity', 'events.event_video +video_opts', 'network.extract',
     'network.colour_map', 'cellview.layers_from_shapes', 'cellview.levels', 'renderer.body_rec_end', 'reg.avi.close', 'sm.run',
     'sm.close', 'cellview.write_video +video_opts', 'strain.triangles', 'network.strain_coupling', 'strain.labels',
     'strain.artifact_score', 'strain.write_video +video_opts'],
    ['X', 'err', 'p', 't', 'tri_means', 'tri_counts', 'stab_shifts', 'stab_score', 'stab_fallback', 'stab_q', 'deform_gamma',
     'deform_fit_r2', 'deform_gain', 'deform_clipped', 'deform_r_before', 'deform_r_after', 'pca_lambda', 'pca_share',
     'pca_temporal', 'pca_rho', 'pca_frame_score', 'pca_frame_r', 'detrend_mean', 'detrend_std', 'detrend_max', 'detrend_corr',
     'residual_round', 'residual_scores', 'residual_scores_round', 'residual_clipped', 'body_mean', 'body_std', 'body_max',
     'body_corr', 'found_points', 'found_scores', 'points', 'point_means', 'point_counts', 'demix_shapes', 'demix_C',
     'demix_dff', 'demix_change', 'roi_points', 'roi_footprints', 'roi_labels', 'roi_counts', 'roi_ring_counts', 'roi_F',
     'roi_Fnp', 'roi_dff', 'roi_seed_fallback', 'ev_g', 'ev_lambda', 'ev_c', 'ev_s', 'ev_binary', 'ev_count_image',
     'ev_sum_image', 'ev_params', 'net_r_events', 'net_r', 'net_labels', 'net_ens_traces', 'net_lead_lag', 'net_lead_r',
     'net_rho', 'net_map', 'net_p_r', 'net_p_map', 'net_rho_max', 'net_sig', 'net_map_sig', 'Xs', 'Xs_std', 'strain_J',
     'strain_l1', 'strain_l2', 'strain_axis', 'strain_rotation', 'strain_body_area', 'net_strain_r', 'strain_cell_J',
     'strain_cell_l1', 'strain_cell_l2', 'strain_artifact_r'],
    ['Cannot read flow stream at noflow*: computing Brox flow in-process', 'Frame 1', 'Frame 2', 'Frame 3',
     'Stabilised (field): 4 patches of 16 px, search 3, 1 passes: 0.0 % fallbacks, mean |shift| 0.000 px',
     'Deformation corrected: gamma 0.500 (fitted, r2 0.750), gains 1.000 .. 1.000 over 1 triangles, 0 values clipped, median '
     '|r| with the area change 0.000 -> 0.000',
     'PCA: 2 components of 3 frames carry 0.2500 0.2500 of the variance; lowest frame score 1.000 at frame 1',
     'Detrended: the excess over the running baseline (half 20, q 10) of 3 frames summed up',
     'Found 1 more points in 1 rounds of the residual video (1 candidates refused, 7 values clipped)',
     'Found 3 points (corr, radius 6) in 3 frames', 'Tracked points: out_points.txt', 'Points found: found.csv',
     'dF/F video: 3 frames in dff.avi', 'Demixed: 3 cells, 6 rounds, last change 0.25',
     'Residual video: 3 frames in res.avi (0 values clipped)', 'ROIs: 3 cells, 9..9 pixels, 0 kept their disc',
     'Events: 3 cells, g 0.900..0.900, 0 events; per pixel g 0.900, lambda 25.5, s_min 51: 0 events',
     'Event video: 3 frames in ev.avi', 'Network: 1 ensembles of 2 cells, 1 cells alone, 64 pixels mapped',
     'Null: ensemble 0: the largest rho of 5 shifted traces 0.0000, 0 significant pixels', 'Ensemble map: map.png',
     'Cells video: 1 (pixel, cell) entries beyond two cells per pixel are not drawn', 'Registered video: 3 frames in reg.avi',
     'Smoothed track: Xs, Xs_std (3 frames)', 'Cells video: 3 frames (smoothed states) in cells.avi',
     'Strain: 1 triangles, body area 1.0000 .. 1.0000 of the rest area', 'Strain video: 3 frames (J) in strain.avi',
     'Finished: 3 frames, states in out.npz'])
RUNS["given_points_rois_resummarize"] = (
    ['in.npy', 'noflow', 'out.npz', '--points', 'p.csv', '--rois', '--resummarize', '--stabilize', '--cells-video', 'cells.avi',
     '--strain'],
    {},
    ['deepio.load_deep', 'VideoStream(in.npy)', 'DistMesh', 'distmesh.createMesh', 'FlowStream',
     'IteratedMSKalmanFilter(cuda=True)', 'FlowEKFPipeline(Video)', 'renderer.body_map', 'record_bytes',
     'BodyReadout(stats=False, keep=True)', 'pipe.run', 'pipe.close', 'body.results', 'stabilize.stabilize', 'detrend.summary',
     'renderer.body_stats_end', 'body.locate', 'roi.extract', 'cellview.layers_from_labels', 'cellview.levels',
     'renderer.body_rec_end', 'cellview.write_video', 'strain.triangles', 'strain.labels', 'strain.artifact_score'],
    ['X', 'err', 'p', 't', 'tri_means', 'tri_counts', 'points', 'point_means', 'point_counts', 'stab_shifts', 'stab_score',
     'stab_fallback', 'detrend_mean', 'detrend_std', 'detrend_max', 'detrend_corr', 'roi_points', 'roi_footprints',
     'roi_labels', 'roi_counts', 'roi_ring_counts', 'roi_F', 'roi_Fnp', 'roi_dff', 'roi_seed_fallback', 'strain_J', 'strain_l1',
     'strain_l2', 'strain_axis', 'strain_rotation', 'strain_body_area', 'strain_cell_J', 'strain_cell_l1', 'strain_cell_l2',
     'strain_artifact_r'],
    ['Cannot read flow stream at noflow*: computing Brox flow in-process',
     'Warning: point 1 (5.5, 4.5) lies outside the mesh: NaN in every frame', 'Frame 1', 'Frame 2', 'Frame 3',
     'Tracked points: out_points.txt',
     'Stabilised: 4 patches of 16 px, search 3, 1 passes: 0.0 % fallbacks, mean |shift| 0.000 px',
     'Resummarised: 3 frames of the stabilised record summed up', 'ROIs: 2 cells, 9..9 pixels, 0 kept their disc',
     'Cells video: 3 frames (filtered states) in cells.avi', 'Strain: 1 triangles, body area 1.0000 .. 1.0000 of the rest area',
     'Finished: 3 frames, states in out.npz'])
RUNS["record_over_budget"] = (
    ['in.npy', 'noflow', 'out.npz', '--find-points', '5', '--rois', '--stabilize', '--dff-video', 'dff.avi'],
    {'record': 1152921504606846976},
    ['deepio.load_deep', 'VideoStream(in.npy)', 'DistMesh', 'distmesh.createMesh', 'FlowStream',
     'IteratedMSKalmanFilter(cuda=True)', 'FlowEKFPipeline(Video)', 'renderer.body_map', 'record_bytes',
     'BodyReadout(stats=True, keep=False)', 'pipe.run', 'pipe.close', 'body.results', 'body.summary', 'body.find_points',
     'renderer.body_stats_end', 'read_out'],
    ['X', 'err', 'p', 't', 'tri_means', 'tri_counts', 'body_mean', 'body_std', 'body_max', 'body_corr', 'found_points',
     'found_scores', 'points', 'point_means', 'point_counts'],
    ['Cannot read flow stream at noflow*: computing Brox flow in-process',
     'The registered video takes 1152921504606846976 bytes on the device, --rois-max-gb allows 8589934592: no ROIs, no '
     'stabilisation, the disc read-out instead',
     'No running baseline either: no --detrend, --resummarize or --dff-video', 'Frame 1', 'Frame 2', 'Frame 3',
     'Found 2 points (corr, radius 6) in 3 frames', 'Tracked points: out_points.txt', 'Finished: 3 frames, states in out.npz'])
RUNS["deep_traces_of_points"] = (
    ['in.npy', 'noflow', 'out.npz', '--points', 'p.csv', '--deep-traces', '--deep-offset', '3'],
    {'deep': True},
    ['deepio.load_deep', 'VideoStream(mapped frames)', 'DistMesh', 'distmesh.createMesh', 'FlowStream',
     'IteratedMSKalmanFilter(cuda=True)', 'deepio.DeepSource', 'FlowEKFPipeline(SimpleNamespace)',
     'BodyReadout(stats=False, keep=False)', 'pipe.run', 'pipe.close', 'DeepSource.close', 'stack.close', 'body.results',
     'deepio.open_deep', 'deeptrace.columns', 'deeptrace.run', 'src16.close', 'deeptrace.point_means'],
    ['X', 'err', 'p', 't', 'depth_lo', 'depth_hi', 'depth_gamma', 'depth_clipped', 'tri_means', 'tri_counts', 'points',
     'point_means', 'point_counts', 'deep_point_means', 'deep_offset'],
    ['16-bit input: window 100..4000 (gamma 1) becomes 0..255; 0 pixels below it, 0 above',
     'Cannot read flow stream at noflow*: computing Brox flow in-process',
     'Warning: point 1 (5.5, 4.5) lies outside the mesh: NaN in every frame', 'Frame 1', 'Frame 2', 'Frame 3',
     'Tracked points: out_points.txt', 'Full-depth traces: the discs of 2 points over 3 frames',
     'Finished: 3 frames, states in out.npz'])
RUNS["given_points_demix_deep_traces"] = (
    ['in.npy', 'noflow', 'out.npz', '--points', 'p.csv', '--demix', '--events', '--network', '--deep-traces'],
    {'deep': True},
    ['deepio.load_deep', 'VideoStream(mapped frames)', 'DistMesh', 'distmesh.createMesh', 'FlowStream',
     'IteratedMSKalmanFilter(cuda=True)', 'deepio.DeepSource', 'FlowEKFPipeline(SimpleNamespace)', 'renderer.body_map',
     'record_bytes', 'BodyReadout(stats=False, keep=True)', 'pipe.run', 'pipe.close', 'DeepSource.close', 'stack.close',
     'body.results', 'body.locate', 'demix.extract', 'deepio.open_deep', 'deeptrace.extract', 'src16.close', 'events.noise',
     'events.noise', 'events.estimate_g', 'events.estimate_g', 'events.default_lam', 'events.default_lam',
     'events.default_smin', 'events.default_smin', 'events.deconvolve', 'events.count_image', 'events.binarise',
     'network.coactivity', 'network.extract', 'renderer.body_rec_end'],
    ['X', 'err', 'p', 't', 'depth_lo', 'depth_hi', 'depth_gamma', 'depth_clipped', 'tri_means', 'tri_counts', 'points',
     'point_means', 'point_counts', 'demix_shapes', 'demix_C', 'demix_dff', 'demix_change', 'roi_points', 'roi_footprints',
     'roi_labels', 'roi_counts', 'roi_ring_counts', 'roi_F', 'roi_Fnp', 'roi_dff', 'roi_seed_fallback', 'deep_F_roi',
     'deep_F_np', 'deep_dff', 'deep_offset', 'deep_demix_c', 'ev_g', 'ev_lambda', 'ev_c', 'ev_s', 'ev_binary', 'ev_count_image',
     'ev_sum_image', 'ev_params', 'net_r_events', 'net_r', 'net_labels', 'net_ens_traces', 'net_lead_lag', 'net_lead_r',
     'net_rho', 'net_map'],
    ['16-bit input: window 100..4000 (gamma 1) becomes 0..255; 0 pixels below it, 0 above',
     'Cannot read flow stream at noflow*: computing Brox flow in-process',
     'Warning: point 1 (5.5, 4.5) lies outside the mesh: NaN in every frame', 'Frame 1', 'Frame 2', 'Frame 3',
     'Tracked points: out_points.txt', 'Demixed: 2 cells, 6 rounds, last change 0.25',
     'ROIs: 2 cells, 9..9 pixels, 0 kept their disc', 'Full-depth traces: 2 cells over 3 frames, F_roi 1.0..1.0',
     'Events: 2 cells, g 0.900..0.900, 0 events; per pixel g 0.900, lambda 25.5, s_min 51: 0 events',
     'Network: 1 ensembles of 2 cells, 1 cells alone, 64 pixels mapped', 'Finished: 3 frames, states in out.npz'])
RUNS["flow_files_smooth_avi_screenshots"] = (
    ['in.npy', 'flow', 'out.avi', '-n', 'run', '--smooth', '-c', 'False'],
    {'flow_files': True},
    ['deepio.load_deep', 'VideoStream(in.npy)', 'DistMesh', 'distmesh.createMesh', 'distmesh.size', 'check_budget',
     'FlowStream', 'AviWriter(out.avi)', 'IteratedMSKalmanFilter(cuda=True)', 'RTSSmoother(3)', 'kf.compute', 'kf.screenshots',
     'renderer.view', 'out.avi.write', 'kf.compute', 'kf.screenshots', 'renderer.view', 'out.avi.write', 'kf.compute',
     'kf.screenshots', 'renderer.view', 'out.avi.write', 'out.avi.close', 'sm.run', 'sm.close'],
    ['X', 'err', 'p', 't', 'Xs', 'Xs_std'],
    ['Frame 1', 'Frame 2', 'Frame 3', 'Overlay video: 3 frames in out.avi', 'Smoothed track: Xs, Xs_std (3 frames)',
     'Finished: 3 frames, states in out.avi'])


@pytest.mark.parametrize("name", list(RUNS))
def test_stage_order(name, monkeypatch, tmp_path):
    argv, how, calls, files, lines = RUNS[name]
    got = _run(monkeypatch, tmp_path, argv, **how)
    assert got[0] == calls
    assert got[1] == files
    assert got[2] == lines


def test_defaults_notice_without_arguments(monkeypatch, tmp_path):
    """len(sys.argv) == 1 and no argv handed in: the notice, then the default names"""
    monkeypatch.chdir(tmp_path)
    os.mkdir("video")
    cli, log = _stub(monkeypatch)
    monkeypatch.setattr(sys, "argv", ["run_kalmanfilter.py"])
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert cli.main() == 0
    lines = out.getvalue().splitlines()
    assert lines[0] == "No command line arguments provided, using defaults"
    assert lines[-1] == "Finished: 3 frames, states in ./video/johntest_brightcontrast_short_output.npz"
    assert log[1] == "VideoStream(./video/johntest_brightcontrast_short.npy)"
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert cli.main([]) == 0                                   # (an empty argv handed in: no notice)
    assert "No command line arguments" not in out.getvalue()

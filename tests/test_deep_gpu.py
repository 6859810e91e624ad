"""The device half of the 16-bit input against tests/deep_ref.py and NumPy: k_deep_hist exactly equal to np.bincount (one
pixel, odd sizes, one hot bin, the borders of the range's quarters, several calls, reset, swapped bytes, more frames than a
run); k_deep_map byte for byte (odd pixel counts, 1 x 1, runs, planted values round lo and hi, both byte orders,
thresholds, gamma, pitch and guard bytes, NULL planes, clip counts); the refusals; the device path of deepio against its
host path; the pipeline fed from DeepSource against ArraySource, bit for bit; and the CLI on a 16-bit TIFF."""
import ctypes
import math
import os

import numpy as np
import pytest

import deep_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


class _Stream:
    def __init__(self):
        from hydra_mi import _lib
        self._lib, self.h = _lib, _lib.c_vp()
        _lib.check(_lib.lib().hm_copy_stream_create(0, ctypes.byref(self.h)), "hm_copy_stream_create")

    def sync(self):
        self._lib.check(self._lib.lib().hm_copy_stream_sync(0, self.h), "hm_copy_stream_sync")

    def close(self):
        self._lib.lib().hm_copy_stream_destroy(0, self.h)


def _handle(W, H, run):
    from hydra_mi import deepio
    return deepio._Handle(W, H, run, 0)


# ---- k_deep_hist -------------------------------------------------------------------------------------------------------
BORDERS = [0, 16383, 16384, 32767, 32768, 49151, 49152, 65535]     # the borders of any split of the range into quarters or halves


def _hist_video(kind):
    rng = np.random.default_rng(7)
    if kind == "1x1":
        return np.array([[[40000]]], np.uint16)
    if kind == "17x33":
        return rng.integers(0, 65536, (3, 17, 33)).astype(np.uint16)
    if kind == "hot":
        return np.full((4, 64, 64), 300, np.uint16)               # one bin holds 16 384
    if kind == "borders":
        return np.array(BORDERS, np.uint16).reshape(1, 2, 4)
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["1x1", "17x33", "hot", "borders"])
def test_hist_equals_bincount(hm, kind):
    a = _hist_video(kind)
    F, H, W = a.shape
    want = np.bincount(a.reshape(-1), minlength=65536).astype(np.uint64)
    h = _handle(W, H, 4)
    try:
        hist, n = h.hist_get()
        assert n == 0 and not hist.any()                          # before anything was added
        h.hist_add(a, 0)
        hist, n = h.hist_get()
        assert n == a.size and np.array_equal(hist, want)
        if kind == "hot":
            assert hist[300] == 16384
        h.hist_add(a[:1], 0)                                      # additive over calls
        h.hist_add(a[1:], 0) if F > 1 else h.hist_add(a, 0)
        hist, n = h.hist_get()
        assert n == 2 * a.size + (a.size if F == 1 else 0) and np.array_equal(hist, (3 if F == 1 else 2) * want)
        h.hist_reset()
        hist, n = h.hist_get()
        assert n == 0 and not hist.any()
        h.hist_add(a.byteswap(), 1)                               # big-endian bytes, swap = 1
        hist, n = h.hist_get()
        assert n == a.size and np.array_equal(hist, want)
    finally:
        h.close()


def test_hist_of_more_frames_than_a_run(hm):
    rng = np.random.default_rng(8)
    a = rng.integers(0, 65536, (7, 17, 33)).astype(np.uint16)
    a[3] = rng.integers(1000, 1010, (17, 33))                     # a near-constant frame among them
    h = _handle(33, 17, 3)
    try:
        h.hist_add(a, 0)
        hist, n = h.hist_get()
        assert n == a.size and np.array_equal(hist, np.bincount(a.reshape(-1), minlength=65536).astype(np.uint64))
    finally:
        h.close()


# ---- k_deep_map --------------------------------------------------------------------------------------------------------
LO, HI = 1200, 3800
MAX_RUN = 4


def _map_video(H, W, frames, seed):
    """frames of values round the window, with 0, lo - 1, lo, lo + 1, hi - 1, hi, hi + 1 and 65535 planted"""
    rng = np.random.default_rng(seed)
    a = rng.integers(LO - 300, HI + 300, (frames, H, W)).astype(np.uint16)
    planted = [0, LO - 1, LO, LO + 1, HI - 1, HI, HI + 1, 65535]
    flat = a.reshape(-1)
    if flat.size >= 8:
        at = rng.choice(flat.size, 8, replace=False)
        flat[at] = planted
        flat[0], flat[-1] = LO - 1, HI + 1                        # the run's first and last pixel clip
    else:
        flat[:] = planted[2:2 + flat.size][::-1]
    return a


_REF = {}


def _reference(a, gamma, threshold):
    """deep_ref's planes and clip counts of every frame, computed once per video, gamma and threshold"""
    key = (a.tobytes(), a.shape, gamma, threshold)
    if key not in _REF:
        lut = _REF.setdefault(("lut", gamma), ref.make_lut(LO, HI, gamma))
        planes = [ref.map_frame(f.reshape(-1).tolist(), lut, LO, HI, threshold) for f in a]
        _REF[key] = tuple(np.array([p[i] for p in planes], np.uint8 if i < 3 else np.uint32) for i in range(4))
    return _REF[key]


def _run_map(h, a, swap, threshold, stride, planes=3):
    """hm_deep_map_run_dev into filled buffers -> ([raw, mask, shown][:planes] as (F, n) arrays, clip (F, 2)); every byte
    that is no pixel (between the planes of two frames, GUARD bytes behind the last) is checked to have kept its fill"""
    from hydra_mi.pipeline import DeviceBuffer
    F, H, W = a.shape
    n = H * W
    bufs = [DeviceBuffer((F - 1) * stride + n + GUARD) for _ in range(planes)]
    status = DeviceBuffer(8 * F + GUARD)
    stream = _Stream()
    try:
        for b in bufs + [status]:
            b.upload(np.full(b.nbytes, FILL, np.uint8))
        block = a.byteswap() if swap else a
        h.map_run_dev(block, swap, bufs[0].ptr, bufs[1].ptr if planes > 1 else None, bufs[2].ptr if planes > 2 else None, stride,
                      threshold, status.ptr, stream.h)
        stream.sync()
        assert h.uploaded()[0] == 2 * n * F
        out = []
        for b in bufs:
            raw = b.download(np.empty(b.nbytes, np.uint8))
            pixel = np.zeros(raw.size, bool)
            for i in range(F):
                pixel[i * stride:i * stride + n] = True
            assert (raw[~pixel] == FILL).all(), "bytes outside the frames were written"
            out.append(np.stack([raw[i * stride:i * stride + n] for i in range(F)]))
        st = status.download(np.empty(status.nbytes, np.uint8))
        assert (st[8 * F:] == FILL).all()
        return out, st[:8 * F].view(np.uint32).reshape(F, 2)
    finally:
        stream.close()
        status.close()
        for b in bufs:
            b.close()


@pytest.mark.parametrize("frames", [1, 3, MAX_RUN])
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (17, 33), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_map_equals_the_reference(hm, shape, frames):
    from hydra_mi import deepio
    H, W = shape
    n = H * W
    a = _map_video(H, W, frames, seed=H * 100 + frames)
    h = _handle(W, H, MAX_RUN)
    try:
        for gamma in (1.0, 0.5):
            lut = deepio.make_lut(LO, HI, gamma)
            assert lut.tolist() == _REF.setdefault(("lut", gamma), ref.make_lut(LO, HI, gamma))
            h.set_lut(lut, LO, HI)
            for threshold in (0, 254, 255):
                want = _reference(a, gamma, threshold)
                # dense planes as in the frame ring, both byte orders; then a pitch that is no multiple of anything
                for swap, stride in ((0, n), (1, n), (0, n + 13)):
                    got, clip = _run_map(h, a, swap, threshold, stride)
                    for i in range(3):
                        assert np.array_equal(got[i], want[i]), (gamma, threshold, swap, stride, "raw mask shown".split()[i])
                    assert np.array_equal(clip, want[3]), (gamma, threshold, swap, stride)
            got, clip = _run_map(h, a, 0, 0, n + 8, planes=1)      # no mask, no shown frame
            assert np.array_equal(got[0], _reference(a, gamma, 0)[0]) and np.array_equal(clip, _reference(a, gamma, 0)[3])
    finally:
        h.close()


def test_map_clip_counts(hm):
    from hydra_mi import deepio
    H, W = 17, 33
    n = H * W
    a = _map_video(H, W, 3, seed=1)
    a[1], a[2] = LO - 1, HI + 1                                   # all below, all above
    h = _handle(W, H, 3)
    try:
        h.set_lut(deepio.make_lut(LO, HI), LO, HI)
        got, clip = _run_map(h, a, 0, 9, n)
        assert clip[0].tolist() == [int((a[0] < LO).sum()), int((a[0] > HI).sum())] and min(clip[0]) > 0
        assert clip[1].tolist() == [n, 0] and clip[2].tolist() == [0, n]
        assert not got[0][1].any() and (got[0][2] == 255).all() and not got[1][1].any() and (got[2][2] == 255).all()
        out, c1 = h.map(a[0], 0)                                  # hm_deep_map: one frame, synchronous
        assert np.array_equal(out.reshape(-1), got[0][0]) and c1.tolist() == clip[0].tolist()
        out, c1 = h.map(a[2].byteswap(), 1)
        assert (out == 255).all() and c1.tolist() == [0, n]
    finally:
        h.close()


def test_refusals(hm):
    from hydra_mi import _lib, deepio
    from hydra_mi.pipeline import DeviceBuffer
    L = _lib.lib()
    out = _lib.c_vp()
    assert L.hm_deep_create(0, 0, 5, 1, ctypes.byref(out)) == -1 and b"0x5 outside 1..32767" in L.hm_last_error()
    assert L.hm_deep_create(0, 5, 5, 65, ctypes.byref(out)) == -1 and b"max_run 65 outside 1..64" in L.hm_last_error()
    a = np.zeros((3, 4, 4), np.uint16)
    buf = DeviceBuffer(3 * 16 + GUARD)
    stream = _Stream()
    h = _handle(4, 4, 2)
    try:
        with pytest.raises(RuntimeError, match="code -3.*no table set"):
            h.map_run_dev(a[:1], 0, buf.ptr, None, None, 16, 0, None, stream.h)
        with pytest.raises(RuntimeError, match="code -3.*no table set"):
            h.map(a[0], 0)
        with pytest.raises(RuntimeError, match="lo 7 >= hi 7"):
            h.set_lut(np.zeros(65536, np.uint8), 7, 7)
        with pytest.raises(RuntimeError, match="lo 9 >= hi 7"):
            h.set_lut(np.zeros(65536, np.uint8), 9, 7)
        h.set_lut(deepio.make_lut(1, 2), 1, 2)
        with pytest.raises(RuntimeError, match="3 frames outside 1..max_run = 2"):
            h.map_run_dev(a, 0, buf.ptr, None, None, 16, 0, None, stream.h)
        with pytest.raises(RuntimeError, match="threshold 256 outside 0..255"):
            h.map_run_dev(a[:1], 0, buf.ptr, None, None, 16, 256, None, stream.h)
        with pytest.raises(RuntimeError, match="threshold -1 outside 0..255"):
            h.map_run_dev(a[:1], 0, buf.ptr, None, None, 16, -1, None, stream.h)
        h.map_run_dev(a[:2], 0, buf.ptr, None, None, 16, 255, None, stream.h)       # and the handle works afterwards
        stream.sync()
        assert h.uploaded() == (2 * 2 * 16, 2 * 2 * 16)
    finally:
        h.close()
        stream.close()
        buf.close()


# ---- deepio: the device path equals the host path ----------------------------------------------------------------------
def test_device_path_equals_host_path(hm, tmp_path):
    from hydra_mi import deepio
    rng = np.random.default_rng(5)
    a = rng.integers(800, 5000, (11, 17, 33)).astype(np.uint16)
    a[4, 2:5, 3:9] = 60000
    hist = deepio.histogram(a, device=0, run=4)
    assert hist.dtype == np.uint64 and np.array_equal(hist, deepio.histogram(a, device=None))
    assert np.array_equal(deepio.histogram(a.astype(">u2"), device=0), hist)
    lo, hi = deepio.window(hist, 1000, 990000)                    # a hundredth of 6171 pixels may clip: the burst does
    for gamma in (1.0, 0.5):
        lut = deepio.make_lut(lo, hi, gamma)
        f_dev, c_dev = deepio.map_video(a, lut, lo, hi, device=0, run=4)
        f_host, c_host = deepio.map_video(a, lut, lo, hi, device=None)
        assert np.array_equal(f_dev, f_host) and np.array_equal(c_dev, c_host) and c_host[4, 1] > 0
    from PIL import Image
    path = str(tmp_path / "s.tif")
    ims = [Image.fromarray(p) for p in a]
    ims[0].save(path, format="TIFF", save_all=True, append_images=ims[1:])
    with deepio.TiffStack(path) as st:
        assert np.array_equal(deepio.histogram(st, device=0), hist)
        f_st, c_st = deepio.map_video(st, lut, lo, hi, device=0)
        assert np.array_equal(f_st, f_host) and np.array_equal(c_st, c_host)


# ---- the pipeline fed with 16-bit pixels -------------------------------------------------------------------------------
N, FRAMES, THRESHOLD = 128, 8, 9


@pytest.mark.parametrize("resident", [False, True], ids=["ring", "resident"])
def test_pipeline_from_deep_source_equals_array_source(hm, resident):
    """FlowEKFPipeline from DeepSource against ArraySource(mapped, masks, mapped x masks): states and iteration counts
    bit-equal after every frame; with flow_batch 1 the ring has 6 slots for 8 frames, so slots wrap and the mirror slot is
    used.  The 16-bit video is 40 v + 1000 + noise of the 8-bit test video, so its mapped frames stay close to v and the
    golden mesh of config 1 fits them."""
    from hydra_mi import deepio, kalman, mesh, pipeline, synth
    video, flow = synth.test_data(N, N)
    vid = np.ascontiguousarray(np.moveaxis(video[:, :, :FRAMES], 2, 0))
    noise = np.random.default_rng(3).integers(0, 40, vid.shape)
    deep = (40 * vid.astype(np.int64) + 1000 + noise).astype(np.uint16)
    win = deepio.resolve(deep, None, device=0)
    mapped, clipped = deepio.map_video(deep, win["lut"], win["lo"], win["hi"], device=0)
    assert np.abs(mapped.astype(int) - vid.astype(int)).max() <= 2
    masks = pipeline.threshold_mask(mapped, THRESHOLD)
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "config1_track.npz"))

    def run(source):
        kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), mapped[0], flow[:, :, :, 0], True)
        pipe = pipeline.FlowEKFPipeline(kf, source, flow_batch=1, resident=resident)
        iters = []
        try:
            assert pipe.ring.R == (FRAMES if resident else 6)
            pipe.run(on_frame=lambda k, e: iters.append(tuple(float(e[i]) for i in range(4)) +
                                                        (np.array(kf.state.X, np.float64).tobytes(),)))
            return np.array(kf.state.X, np.float64).copy(), iters, pipe.ring.bytes_uploaded
        finally:
            pipe.close()
            kf.close()

    src = deepio.DeepSource(deep, win["lut"], win["lo"], win["hi"], THRESHOLD, frames=mapped)
    try:
        assert len(src) == FRAMES and src.shape == (N, N)
        Xa, ia, sent = run(src)
        assert np.array_equal(src.clipped, clipped)
    finally:
        src.close()
    Xb, ib, raw = run(pipeline.ArraySource(mapped, masks, mapped * masks))
    assert np.array_equal(Xa, Xb)
    assert len(ia) == FRAMES - 1 and ia == ib
    assert sent == FRAMES * 2 * N * N and raw == 3 * FRAMES * N * N


def test_deep_source_maps_on_demand(hm):
    from hydra_mi import deepio
    a = _map_video(17, 33, 3, seed=9)
    lut = deepio.make_lut(LO, HI)
    src = deepio.DeepSource(a.astype(">u2"), lut, LO, HI, THRESHOLD)
    try:
        fr, mk, sh = src.frame_at(2)
        assert np.array_equal(fr, lut[a[2]]) and np.array_equal(mk, fr > THRESHOLD) and np.array_equal(sh, mk * fr)
    finally:
        src.close()


def test_cli_takes_a_16_bit_tiff(hm, tmp_path, monkeypatch, capsys):
    """run_kalmanfilter.py v.tif none out.npz gives the X of run_kalmanfilter.py v.npy none out.npz, v.npy the mapped frames"""
    import sys
    from PIL import Image
    from hydra_mi import pipeline, synth
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_kalmanfilter as cli
    n, F = 96, 5
    video, masks, c, r = synth.disk_video(n, F, "translate_leftup", 0)
    deep = (40 * video.astype(np.int64) + 1000 + np.random.default_rng(4).integers(0, 40, video.shape)).astype(np.uint16)
    monkeypatch.chdir(tmp_path)
    ims = [Image.fromarray(p) for p in deep]
    ims[0].save("v.tif", format="TIFF", save_all=True, append_images=ims[1:])
    mapped = pipeline.load_video("v.tif")
    assert mapped.dtype == np.uint8 and mapped.shape == video.shape
    np.save("v.npy", mapped)
    assert cli.main(["v.tif", "none", "tif.npz", "-s", "14"]) == 0
    assert "16-bit input: window" in capsys.readouterr().out
    assert cli.main(["v.npy", "none", "npy.npz", "-s", "14"]) == 0
    out = np.load("tif.npz")
    assert np.array_equal(out["X"], np.load("npy.npz")["X"])
    assert math.isfinite(float(out["X"].sum()))
    h = np.bincount(deep.reshape(-1), minlength=65536)
    lo, hi = ref.window(h.tolist())
    assert (int(out["depth_lo"]), int(out["depth_hi"]), float(out["depth_gamma"])) == (lo, hi, 1.0)
    assert out["depth_clipped"].shape == (F, 2)
    assert np.array_equal(out["depth_clipped"], np.stack([(deep < lo).sum((1, 2)), (deep > hi).sum((1, 2))], 1))
    assert "depth_lo" not in np.load("npy.npz").files
    # with a readout the depth_* arrays stand beside its arrays; a threshold off the 8-bit scale is refused before tracking
    assert cli.main(["v.tif", "none", "reg.npz", "-s", "14", "--registered", "reg.avi", "--depth-range", "%d,%d" % (lo, hi)]) == 0
    reg = np.load("reg.npz")
    assert {"tri_means", "depth_lo", "depth_clipped"} <= set(reg.files) and np.array_equal(reg["X"], out["X"])
    with pytest.raises(SystemExit):
        cli.main(["v.tif", "none", "bad.npz", "-s", "14", "-t", "300"])

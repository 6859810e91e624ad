"""The device's JPEG encoder against the restatement of tests/mjpeg_ref.py: hm_mjpeg_encode and hm_mjpeg_encode_dev give
exactly its bytes at every shape of mjpeg_ref.cases() (block edges, restart intervals, more blocks in an interval than a
workgroup has threads, the largest symbols); no state is left between frames; a `cap` that is too small writes nothing;
and a pipeline run with an MJPEG video leaves the track as it is without one."""
import ctypes
import io
import os

import numpy as np
import pytest

import mjpeg_ref

pytestmark = pytest.mark.gpu

CASES = mjpeg_ref.cases()


def _pinned_u8(lib, n):
    p = lib.c_vp()
    lib.check(lib.lib().hm_host_alloc(n, ctypes.byref(p)), "hm_host_alloc")
    return p, np.ctypeslib.as_array(ctypes.cast(p.value, ctypes.POINTER(ctypes.c_uint8)), shape=(n,))


def _encode_dev(hm, enc, frame, cap=None, pinned_out=False, guard=64):
    """-> (size word, the cap bytes of `out`, the guard bytes behind them), through hm_mjpeg_encode_dev on a copy stream;
    the size word is page-locked, `out` device or page-locked memory"""
    from hydra_mi import _lib
    from hydra_mi.pipeline import DeviceBuffer
    L = _lib.lib()
    cap = enc.max_stream if cap is None else cap
    stream = _lib.c_vp()
    _lib.check(L.hm_copy_stream_create(0, ctypes.byref(stream)), "hm_copy_stream_create")
    d_frame = DeviceBuffer(frame.nbytes)
    d_frame.upload(frame)
    word_p, word = _pinned_u8(_lib, 16)
    fill = np.full(cap + guard, 0xA5, np.uint8)
    try:
        if pinned_out:
            out_p, out = _pinned_u8(_lib, cap + guard)
            out[:] = fill
            enc.encode_dev(d_frame.ptr, out_p.value, cap, word_p.value, stream)
            _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
            got = out.copy()
            L.hm_host_free(out_p)
        else:
            d_out = DeviceBuffer(cap + guard)
            d_out.upload(fill)
            enc.encode_dev(d_frame.ptr, d_out.ptr, cap, word_p.value, stream)
            _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
            got = d_out.download(np.empty(cap + guard, np.uint8))
            d_out.close()
        size = int(word[:4].view(np.uint32)[0])
    finally:
        L.hm_host_free(word_p)
        d_frame.close()
        L.hm_copy_stream_destroy(0, stream)
    return size, got[:cap], got[cap:]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_bytes_equal_the_restatement(hm, name):
    from hydra_mi.videoio import MjpegEncoder
    _, frame, q, rr = next(c for c in CASES if c[0] == name)
    ref, _ = mjpeg_ref.reference(name)
    ch = 1 if frame.ndim == 2 else 3
    enc = MjpegEncoder(frame.shape[1], frame.shape[0], ch, q, rr)
    try:
        hdr = len(enc.header)
        assert enc.header == ref[:hdr]
        got = enc.encode(frame)
        assert len(got) == len(ref), (len(got), len(ref))
        assert got == ref, "first difference at byte %d" % next(i for i in range(len(ref)) if got[i] != ref[i])
        for pinned in (False, True):
            size, out, guard = _encode_dev(hm, enc, frame, pinned_out=pinned)
            assert size == len(ref) - hdr
            assert out[:size].tobytes() == ref[hdr:]
            assert (out[size:] == 0xA5).all() and (guard == 0xA5).all()
    finally:
        enc.close()


def test_no_state_is_left_between_frames(hm):
    from hydra_mi.videoio import MjpegEncoder
    rng = np.random.default_rng(7)
    for W, H, ch in ((61, 45, 3), (24, 80, 1)):
        enc = MjpegEncoder(W, H, ch, 90, 1)
        try:
            shape = (H, W, 3) if ch == 3 else (H, W)
            A = rng.integers(0, 256, shape, dtype=np.uint8)
            B = np.full(shape, 255, np.uint8) - A // 2
            a1, b1, a2 = enc.encode(A), enc.encode(B), enc.encode(A)
            assert a1 == a2 and a1 != b1
            assert a1 == mjpeg_ref.encode(A, 90, 1)[0] and b1 == mjpeg_ref.encode(B, 90, 1)[0]
        finally:
            enc.close()


def test_cap_one_short_writes_nothing_and_exact_cap_succeeds(hm):
    from hydra_mi.videoio import MjpegEncoder
    name = "edge_61x45_c3"
    _, frame, q, rr = next(c for c in CASES if c[0] == name)
    ref, _ = mjpeg_ref.reference(name)
    enc = MjpegEncoder(61, 45, 3, q, rr)
    try:
        hdr = len(enc.header)
        n = len(ref) - hdr
        size, out, guard = _encode_dev(hm, enc, frame, cap=n - 1)
        assert size == n                                           # the word says what it would have taken
        assert (out == 0xA5).all() and (guard == 0xA5).all()       # and nothing was written, before cap or past it
        size, out, guard = _encode_dev(hm, enc, frame, cap=n)
        assert size == n and out.tobytes() == ref[hdr:] and (guard == 0xA5).all()
        with pytest.raises(RuntimeError, match=r"%d \+ %d bytes, the buffer has %d" % (hdr, n, len(ref) - 1)):
            enc.encode(frame, cap=len(ref) - 1)
        assert enc.encode(frame, cap=len(ref)) == ref
    finally:
        enc.close()


def _psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return 10 * np.log10(255.0 ** 2 / max(np.mean(d * d), 1e-12))


def _pil(frame, quality):
    """the frame through PIL's encoder with our tables, no subsampling, a restart marker per row -> decoded"""
    from PIL import Image
    from hydra_mi.videoio import decode_jpeg
    q = mjpeg_ref.quant_tables(quality)
    buf = io.BytesIO()
    if frame.ndim == 2:
        Image.fromarray(frame).save(buf, "JPEG", qtables=[q[0]], restart_marker_rows=1)
    else:
        Image.fromarray(frame[:, :, ::-1].copy()).save(buf, "JPEG", qtables=q, subsampling=0, restart_marker_rows=1)
    return decode_jpeg(buf.getvalue())


def test_pipeline_run_with_mjpeg_video(hm, tmp_path):
    """BASELINE config 1 (128 x 128): the track is bit-equal with and without the video, the file has a chunk per frame,
    every decoded frame is within a quarter of PIL's step from quality 85 to 90 of PIL's own coding of the same run's raw
    frame, and a registered video is single-component."""
    from hydra_mi import body, kalman, mesh, pipeline, synth, videoio
    n, frames, quality = 128, 5, 90
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "config1_track.npz"))
    video, flow = synth.test_data(n, n)
    vid = np.ascontiguousarray(np.moveaxis(video[:, :, :frames], 2, 0))
    masks = (vid > 0).astype(np.uint8)

    def run(codec, registered=False):
        kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), vid[0], flow[:, :, :, 0], True)
        pipe = pipeline.FlowEKFPipeline(kf, vid, masks, flow_batch=2)
        kw = {}
        path = reg = None
        if codec is not None:
            path = str(tmp_path / ("%s.avi" % codec))
            kw["video"] = videoio.AviWriter(path, n, n, codec=codec, quality=quality)
        if registered:
            reg = str(tmp_path / "reg.avi")
            kw["body"] = body.BodyReadout(kf, video=videoio.AviWriter(reg, n, n, codec="mjpeg", quality=quality, channels=1))
        try:
            pipe.run(**kw)
            X = np.array(kf.state.X, np.float64).copy()
        finally:
            pipe.close()
            for w in (kw.get("video"), kw["body"].video if "body" in kw else None):
                if w is not None:
                    w.close()
            kf.close()
        return X, path, reg

    X0, _, _ = run(None)
    Xr, raw_path, _ = run("raw")
    Xm, mj_path, reg_path = run("mjpeg", registered=True)
    assert np.array_equal(X0, Xr) and np.array_equal(X0, Xm)
    raw, mj = videoio.read_avi(raw_path), videoio.read_avi(mj_path)
    assert len(raw) == len(mj) == frames - 1
    for r, m in zip(raw, mj):
        assert m.shape == (n, n, 3)
        ours, p90, p85 = _psnr(m, r), _psnr(_pil(r, quality), r), _psnr(_pil(r, quality - 5), r)
        print("mjpeg %.3f dB, PIL %.3f dB, PIL at 85 %.3f dB" % (ours, p90, p85))
        assert p90 - ours <= 0.25 * (p90 - p85)
    reg = videoio.read_avi(reg_path)
    assert len(reg) == frames - 1 and all(f.shape == (n, n) for f in reg)


def test_cli_writes_mjpeg_videos(hm, tmp_path, monkeypatch):
    """run_kalmanfilter.py ... out.avi --video-codec mjpeg --registered reg.avi: both files decode frame by frame, the
    overlay with three components and the registered video with one, and the track is that of the raw run"""
    import sys
    from hydra_mi import synth, videoio
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_kalmanfilter as cli
    n, F = 96, 5
    video, masks, c, r = synth.disk_video(n, F, "translate_leftup", 0)
    np.save(str(tmp_path / "video.npy"), video)
    monkeypatch.chdir(tmp_path)
    assert cli.main(["video.npy", "none", "raw.avi", "-s", "14", "--registered", "raw_reg.avi"]) == 0
    assert cli.main(["video.npy", "none", "out.avi", "-s", "14", "--registered", "reg.avi", "--video-codec", "mjpeg",
                     "--video-quality", "95"]) == 0
    assert np.array_equal(np.load("raw.avi.npz")["X"], np.load("out.avi.npz")["X"])
    out, reg = videoio.read_avi("out.avi"), videoio.read_avi("reg.avi")
    raw, raw_reg = videoio.read_avi("raw.avi"), videoio.read_avi("raw_reg.avi")
    assert len(out) == len(reg) == len(raw) == len(raw_reg) == F - 1
    assert os.path.getsize("reg.avi") < os.path.getsize("out.avi") < os.path.getsize("raw.avi")
    for o, g, ro, rg in zip(out, reg, raw, raw_reg):
        assert o.shape == (n, n, 3) and g.shape == (n, n)
        assert _psnr(o, ro) > 30 and _psnr(g, rg[:, :, 0]) > 30          # the same pictures (the rule itself: the test above)


def test_write_dev_and_a_stream_larger_than_the_pinned_room(hm, tmp_path):
    """AviWriter.write_dev appends the restatement's file for a frame that never left the device, and a stream that does
    not fit the page-locked room of a slot (MjpegSlots(room=)) arrives through ordinary memory as the same bytes"""
    from hydra_mi import _lib, videoio
    from hydra_mi.pipeline import DeviceBuffer
    name = "noise_q100"
    _, frame, q, rr = next(c for c in CASES if c[0] == name)
    ref, _ = mjpeg_ref.reference(name)
    L = _lib.lib()
    path = str(tmp_path / "dev.avi")
    stream = _lib.c_vp()
    _lib.check(L.hm_copy_stream_create(0, ctypes.byref(stream)), "hm_copy_stream_create")
    d_frame = DeviceBuffer(frame.nbytes)
    d_frame.upload(frame)
    w = videoio.AviWriter(path, frame.shape[1], frame.shape[0], codec="mjpeg", quality=q, restart_rows=rr)
    slots = videoio.MjpegSlots(w.encoder, 1, 0, room=256)
    d_out = DeviceBuffer(slots.cap)
    try:
        with pytest.raises(ValueError, match="frame of shape"):
            w.write(frame[:, :, 0])
        w.write_dev(d_frame.ptr, stream)
        assert slots.room == 256 < len(ref)
        w.encoder.encode_dev(d_frame.ptr, d_out.ptr, slots.cap, slots.size_word(0), stream)
        _lib.check(L.hm_copy_stream_sync(0, stream), "hm_copy_stream_sync")
        slots.finish(0, d_out.ptr, w)
        w.write(frame)
        assert w.frames == 3
    finally:
        w.close()
        slots.close()
        d_out.close()
        d_frame.close()
        L.hm_copy_stream_destroy(0, stream)
    assert open(path, "rb").read().count(ref) == 3
    back = videoio.read_avi(path)
    assert len(back) == 3 and all(np.array_equal(b, videoio.decode_jpeg(ref)) for b in back)

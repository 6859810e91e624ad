"""The device's JPEG decoder against the restatement of tests/mjpeg_dec_ref.py (which test_mjpeg_dec_cpu.py holds to PIL's
libjpeg bit for bit): hm_mjpeg_decode and hm_mjpeg_decode_run_dev give exactly its bytes through the host and the device
entropy path on every file of mjpeg_dec_cases; the three planes, pitch and guard bytes; no state between frames; bad
intervals; the encoder's files read back; load_video of an .avi; the pipeline fed from AviSource against ArraySource,
bit for bit; and the CLI on an .avi."""
import ctypes
import math
import os

import numpy as np
import pytest

import mjpeg_dec_cases as cases
import mjpeg_dec_ref as ref
import mjpeg_ref

pytestmark = pytest.mark.gpu

FILES = cases.small_files() + cases.large_files()                 # every file of the CPU test, the structural shapes among them
assert {k for k, _ in cases.structural_files()} <= {k for k, _ in FILES}
GUARD = 64


class _Stream:
    def __init__(self):
        from hydra_mi import _lib
        self._lib, self.h = _lib, _lib.c_vp()
        _lib.check(_lib.lib().hm_copy_stream_create(0, ctypes.byref(self.h)), "hm_copy_stream_create")

    def sync(self):
        self._lib.check(self._lib.lib().hm_copy_stream_sync(0, self.h), "hm_copy_stream_sync")

    def close(self):
        self._lib.lib().hm_copy_stream_destroy(0, self.h)


def _run(dec, chunks, threshold=0, pitch=None, planes=3):
    """hm_mjpeg_decode_run_dev into 0xA5-filled buffers -> ([frames], [masks] | None, [shown] | None, status words); every
    byte that is no pixel (row padding, 64 bytes between frames and behind the last) is checked to have kept its fill"""
    from hydra_mi.pipeline import DeviceBuffer
    W, H, n = dec.width, dec.height, len(chunks)
    pitch = W if pitch is None else pitch
    stride = pitch * H + GUARD
    bufs = [DeviceBuffer(n * stride + GUARD) for _ in range(planes)]
    status = DeviceBuffer(4 * n + GUARD)
    stream = _Stream()
    try:
        for b in bufs:
            b.upload(np.full(b.nbytes, 0xA5, np.uint8))
        status.upload(np.full(status.nbytes, 0xA5, np.uint8))
        dec.decode_run_dev(chunks, bufs[0].ptr, bufs[1].ptr if planes > 1 else None, bufs[2].ptr if planes > 2 else None,
                           stride, pitch, threshold, status.ptr, stream.h)
        stream.sync()
        out = []
        for b in bufs:
            raw = b.download(np.empty(b.nbytes, np.uint8))
            pixel = np.zeros(raw.size, bool)
            frames = []
            for i in range(n):
                rows = np.lib.stride_tricks.as_strided(raw[i * stride:], (H, W), (pitch, 1))
                frames.append(rows.copy())
                for y in range(H):
                    pixel[i * stride + y * pitch:i * stride + y * pitch + W] = True
            assert (raw[~pixel] == 0xA5).all(), "bytes outside the frames were written"
            out.append(frames)
        st = status.download(np.empty(status.nbytes, np.uint8))
        assert (st[4 * n:] == 0xA5).all()
        return out[0], out[1] if planes > 1 else None, out[2] if planes > 2 else None, st[:4 * n].view(np.uint32).copy()
    finally:
        stream.close()
        status.close()
        for b in bufs:
            b.close()


@pytest.mark.parametrize("key,data", FILES, ids=[k for k, _ in FILES])
def test_device_bytes_equal_the_restatement(hm, key, data):
    from hydra_mi.videoio import MjpegDecoder
    want, _coef, _bad, g = ref.reference(key, data)
    for entropy in ("host", "device") if g["ri"] else ("host",):
        dec = MjpegDecoder(g["W"], g["H"], 2, entropy=entropy)
        try:
            got = dec.decode(data)
            assert dec.last_bad == 0
            assert np.array_equal(got, want), (entropy, "largest difference %d" % np.abs(got.astype(int) - want).max())
            frames, masks, shown, status = _run(dec, [data], threshold=9)
            assert status.tolist() == [0]
            assert np.array_equal(frames[0], want), entropy
            assert np.array_equal(masks[0], (want > 9).astype(np.uint8)) and np.array_equal(shown[0], (want > 9) * want)
        finally:
            dec.close()


def _files_61x45():
    a = [cases.image(61, 45, 3), cases.image(61, 45, 3)[::-1].copy(), np.random.default_rng(5).integers(0, 256, (45, 61, 3), dtype=np.uint8)]
    return [("run_a", cases.pil_save(a[0], quality=90, subsampling=2, restart_marker_rows=1)),      # 4:2:0 with DRI
            ("run_b", cases.pil_save(a[1], quality=50, subsampling=0)),                               # 4:4:4 without
            ("run_c", cases.pil_save(a[2][:, :, 0].copy(), quality=90, restart_marker_blocks=3))]    # grey, intervals of 3


@pytest.mark.parametrize("entropy", ["auto", "host", "device"])
def test_a_run_of_different_frames_with_and_without_dri(hm, entropy):
    """three frames of different content, sampling and restart interval in one call; with "auto" and the switch-over tuned
    down to 3 intervals the frame without DRI takes the host path and the two with DRI (3 and 16 intervals) the device path,
    in the same launches"""
    from hydra_mi.videoio import MjpegDecoder
    files = _files_61x45()
    want = [ref.reference(k, d)[0] for k, d in files]
    dec = MjpegDecoder(61, 45, 3, entropy=entropy)
    dec.tune("auto_intervals", 3)
    try:
        for order in ((0, 1, 2), (1, 2), (2, 0, 1)):
            frames, _, _, status = _run(dec, [files[i][1] for i in order], planes=1)
            assert not status.any()
            for got, i in zip(frames, order):
                assert np.array_equal(got, want[i]), (order, i)
        with pytest.raises(RuntimeError, match="4 frames outside 1..max_run = 3"):
            _run(dec, [files[0][1]] * 4, planes=1)
    finally:
        dec.close()


@pytest.mark.parametrize("threshold", [0, 9, 255])
def test_the_three_planes_pitch_and_guards(hm, threshold):
    from hydra_mi.pipeline import threshold_mask
    from hydra_mi.videoio import MjpegDecoder
    files = _files_61x45()
    want = [ref.reference(k, d)[0] for k, d in files]
    dec = MjpegDecoder(61, 45, 3)
    try:
        for pitch in (61, 64, 77, 128):                           # dense and odd (bytes), multiples of 4 (words) with padding
            frames, masks, shown, _ = _run(dec, [d for _, d in files], threshold, pitch)
            for i in range(3):
                m = threshold_mask(want[i], threshold)
                assert np.array_equal(frames[i], want[i]) and np.array_equal(masks[i], m) and np.array_equal(shown[i], m * want[i])
        frames, masks, shown, _ = _run(dec, [d for _, d in files], threshold, 64, planes=1)      # mask and shown NULL
        assert masks is None and shown is None and all(np.array_equal(frames[i], want[i]) for i in range(3))
        with pytest.raises(RuntimeError, match="row pitch of 60"):
            _run(dec, [files[0][1]], threshold, 60)
    finally:
        dec.close()


def test_no_state_between_frames(hm):
    from hydra_mi.videoio import MjpegDecoder
    (_, a), (_, b), _ = _files_61x45()
    for entropy in ("host", "device"):
        if entropy == "device":                                   # (both with DRI for the device path)
            b = cases.pil_save(cases.image(61, 45, 1)[::-1].copy(), quality=30, restart_marker_rows=2)
        dec, fresh = MjpegDecoder(61, 45, 1, entropy=entropy), MjpegDecoder(61, 45, 1, entropy=entropy)
        try:
            first, second, third = dec.decode(a), dec.decode(b), dec.decode(a)
            assert np.array_equal(first, third) and np.array_equal(first, fresh.decode(a))
            assert np.array_equal(first, ref.decode(a)[0]) and np.array_equal(second, ref.decode(b)[0])
        finally:
            dec.close()
            fresh.close()


def test_bad_intervals_on_the_device_path(hm):
    """the four malformed streams of the CPU test (tools/mjpeg_dec_check.cpp has walked the same routine over such input
    under the sanitizers): the status word counts the bad interval, its blocks from the bad one on are 128, the other
    intervals equal the restatement, nothing outside the frame is written, and the next clean frame is right"""
    from hydra_mi.videoio import MjpegDecoder
    clean, streams = cases.malformed()
    want_clean = ref.decode(clean)[0]
    for entropy in ("device", "host"):
        dec = MjpegDecoder(32, 32, 2, entropy=entropy)
        try:
            for name, data in streams:
                want, nbad = ref.decode(data)
                assert nbad == 1
                frames, _, _, status = _run(dec, [data, clean])
                assert status.tolist() == [1, 0], (entropy, name)
                assert np.array_equal(frames[0], want), (entropy, name)
                assert (frames[0][8:16, 24:32] == 128).all()                          # the interval's last block
                assert np.array_equal(frames[0][:8], want_clean[:8]) and np.array_equal(frames[0][16:], want_clean[16:])
                assert np.array_equal(frames[1], want_clean)
                with pytest.raises(RuntimeError, match="1 bad restart intervals"):
                    dec.decode(data)
                assert np.array_equal(dec.decode(data, strict=False), want) and dec.last_bad == 1
                assert np.array_equal(dec.decode(clean), want_clean) and dec.last_bad == 0
        finally:
            dec.close()


@pytest.mark.parametrize("name", ["edge_61x45_c3", "edge_61x45_c1", "restart_24x80_r3", "noise_q100"])
def test_round_trip_with_the_device_encoder(hm, name):
    from hydra_mi.videoio import MjpegDecoder, MjpegEncoder
    _, frame, q, rr = next(c for c in mjpeg_ref.cases() if c[0] == name)
    enc = MjpegEncoder(frame.shape[1], frame.shape[0], 1 if frame.ndim == 2 else 3, q, rr)
    dec = MjpegDecoder(frame.shape[1], frame.shape[0])
    try:
        data = enc.encode(frame)
        assert np.array_equal(dec.decode(data), cases.pil_grey(data))
    finally:
        enc.close()
        dec.close()


def _write_avi(path, files, W, H):
    from hydra_mi import videoio
    with videoio.AviWriter(path, W, H, codec="mjpeg", channels=1) as w:
        for data in files:
            w.write_chunk(data)


def test_load_video_of_an_avi(hm, tmp_path):
    from hydra_mi.pipeline import load_video
    frames = [np.roll(cases.image(61, 45, 1), 3 * k, axis=1) for k in range(11)]                 # more than a run of 8
    files = [mjpeg_ref.encode(f, 90, 1)[0] if k % 2 else cases.pil_save(f, quality=90) for k, f in enumerate(frames)]
    want = np.stack([ref.reference("load_%d" % k, d)[0] for k, d in enumerate(files)])
    path = str(tmp_path / "x.avi")
    _write_avi(path, files, 61, 45)
    got = load_video(path)
    assert got.dtype == np.uint8 and got.shape == (11, 45, 61) and np.array_equal(got, want)
    assert np.array_equal(load_video(path, gray=False), want)
    np.save(str(tmp_path / "x.npy"), want)
    assert np.array_equal(load_video(str(tmp_path / "x.npy")), got)
    bad = str(tmp_path / "bad.avi")
    _write_avi(bad, [files[0], cases.malformed()[1][0][1]], 61, 45)
    with pytest.raises(RuntimeError, match="32x32 for a decoder of 61x45"):
        load_video(bad)


# ---- the pipeline fed with JPEG bytes ------------------------------------------------------------------------------------------
N, FRAMES, THRESHOLD = 128, 8, 9
DESC_BYTES = 5608                                                 # HM_MJPEG_DESC_BYTES


def _pipeline_video(tmp_path, kind):
    """the 128 x 128 test video (the configuration of test_mjpeg_gpu.py's pipeline test, eight frames) as an MJPEG AVI ->
    (path, decoded frames, bytes each frame sends over the bus, flow)"""
    from hydra_mi import synth, videoio
    video, flow = synth.test_data(N, N)
    vid = np.ascontiguousarray(np.moveaxis(video[:, :, :FRAMES], 2, 0))
    path = str(tmp_path / ("%s.avi" % kind))
    if kind == "rows1":                                           # this library's encoder: a DRI, run on the device entropy path
        with videoio.AviWriter(path, N, N, codec="mjpeg", channels=1, quality=95, restart_rows=1) as w:
            for f in vid:
                w.write(f)
    else:                                                         # PIL without restart markers: the host entropy path
        _write_avi(path, [cases.pil_save(f, quality=95) for f in vid], N, N)
    with videoio.AviReader(path) as r:
        info = videoio.mjpeg_probe(r.chunk(0))
        assert (info["ri"] != 0) == (kind == "rows1")
        # what hm_mjpeg_decode_run_dev queues host-to-device per frame (include/hydra_mi.h, hm_mjpeg_dec_uploaded): a
        # descriptor, then the file rounded up to 16 bytes and 12 bytes per interval (device entropy path) or 128 bytes
        # of coefficients per luma block (host entropy path)
        sizes = []
        for f in range(len(r)):
            i = videoio.mjpeg_probe(r.chunk(f))
            sizes.append(DESC_BYTES + ((len(r.chunk(f)) + 15) // 16 * 16 + 12 * i["intervals"] if kind == "rows1"
                                       else 128 * i["mcus"] * i["hs"] * i["vs"]))
        decoded = np.stack([cases.pil_grey(bytes(r.chunk(f))) for f in range(len(r))])
    return path, decoded, sizes, flow


@pytest.mark.parametrize("resident", [False, True], ids=["ring", "resident"])
@pytest.mark.parametrize("kind", ["rows1", "pil"])
def test_pipeline_from_avi_source_equals_array_source(hm, tmp_path, kind, resident):
    """FlowEKFPipeline from AviSource against ArraySource(decoded, masks, decoded x masks): states and iteration counts
    bit-equal
    after every frame (the error tuple holds the iteration count); with flow_batch 1 the ring has 6 slots for 8 frames, so slots wrap and the mirror slot is used"""
    from hydra_mi import kalman, mesh, pipeline, videoio
    path, decoded, sizes, flow = _pipeline_video(tmp_path, kind)
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "config1_track.npz"))
    masks = pipeline.threshold_mask(decoded, THRESHOLD)

    def run(source):
        kf = kalman.IteratedMSKalmanFilter(mesh.Mesh(g["p"], g["t"], 15.0), decoded[0], flow[:, :, :, 0], True)
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

    src = videoio.AviSource(path, THRESHOLD, frames=decoded, entropy="device" if kind == "rows1" else "host")
    try:
        assert len(src) == FRAMES and src.shape == (N, N)
        Xa, ia, sent = run(src)
    finally:
        src.close()
    Xb, ib, raw = run(pipeline.ArraySource(decoded, masks, decoded * masks))
    assert np.array_equal(Xa, Xb)
    assert len(ia) == FRAMES - 1 and ia == ib
    print("%s: %d bytes over the bus for %d raw" % (kind, sent, raw))
    assert sent == sum(sizes) and raw == 3 * FRAMES * N * N
    if kind == "pil":                                             # the host path sends coefficients, 2 bytes a pixel, not the file
        assert sent == FRAMES * (DESC_BYTES + 2 * N * N)


def test_avi_source_decodes_on_demand(hm, tmp_path):
    from hydra_mi import videoio
    path, decoded, _, _ = _pipeline_video(tmp_path, "rows1")
    src = videoio.AviSource(path, THRESHOLD)
    try:
        fr, mk, sh = src.frame_at(5)
        assert np.array_equal(fr, decoded[5]) and np.array_equal(mk, decoded[5] > THRESHOLD) and np.array_equal(sh, mk * fr)
    finally:
        src.close()


def test_cli_takes_an_avi(hm, tmp_path, monkeypatch):
    """run_kalmanfilter.py v.avi none out.npz gives the X of run_kalmanfilter.py v.npy none out.npz, v.npy the decoded frames"""
    import sys
    from hydra_mi import synth, videoio
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run_kalmanfilter as cli
    n, F = 96, 5
    video, masks, c, r = synth.disk_video(n, F, "translate_leftup", 0)
    monkeypatch.chdir(tmp_path)
    with videoio.AviWriter("v.avi", n, n, codec="mjpeg", channels=1, quality=95) as w:
        for f in video:
            w.write(f)
    np.save("v.npy", np.stack(videoio.read_avi("v.avi")))                  # (PIL's decode: the frames the device gives)
    assert cli.main(["v.avi", "none", "avi.npz", "-s", "14"]) == 0
    assert cli.main(["v.npy", "none", "npy.npz", "-s", "14"]) == 0
    assert np.array_equal(np.load("avi.npz")["X"], np.load("npy.npz")["X"])
    assert math.isfinite(float(np.load("avi.npz")["X"].sum()))

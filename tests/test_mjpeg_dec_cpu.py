"""CPU checks of the Motion-JPEG decoder (include/hydra_mi.h, "Motion-JPEG, decoding"): the restatement
(tests/mjpeg_dec_ref.py) against PIL's libjpeg bit for bit; the library's host parser and host entropy path against the
restatement (coefficients and interval tables); every refusal by name; bad intervals; AviReader on this library's files
and on a container assembled from the AVI rules; and tools/mjpeg_dec_check.cpp, the parser and the shared entropy routine
under the address and undefined-behaviour sanitizers on every prefix and every bit flip of two small files."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import mjpeg_dec_cases as cases
import mjpeg_dec_ref as ref
import mjpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = cases.small_files()
LARGE = cases.large_files()


def _ids(files):
    return [k for k, _ in files]


# ---- the restatement is libjpeg ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,data", SMALL + LARGE, ids=_ids(SMALL + LARGE))
def test_restatement_equals_pil(key, data):
    frame, _coef, bad, _g = ref.reference(key, data)
    assert bad == []
    want = cases.pil_grey(data)
    assert frame.shape == want.shape
    assert np.array_equal(frame, want), "largest difference %d" % np.abs(frame.astype(int) - want).max()


def test_luma_plane_is_not_gray_of_clamped_colours():
    """the rule 'the grey of a colour JPEG is its luma plane' matters: on saturated noise BGR2GRAY of the decoded colours
    differs from it by far more than rounding (the colour conversion clamps), on a smooth image by rounding at most"""
    from hydra_mi.pipeline import to_gray
    from hydra_mi.videoio import decode_jpeg
    noise = cases.pil_save(np.random.default_rng(1).integers(0, 256, (45, 61, 3), dtype=np.uint8), quality=90, subsampling=0)
    smooth = cases.pil_save(mjpeg_ref.smooth_image(61, 45, 3) // 2 + 64, quality=90, subsampling=0)
    d_noise = np.abs(to_gray(decode_jpeg(noise)).astype(int) - ref.decode(noise)[0]).max()
    d_smooth = np.abs(to_gray(decode_jpeg(smooth)).astype(int) - ref.decode(smooth)[0]).max()
    print("luma plane against to_gray of the decoded colours: noise %d, smooth in-gamut %d" % (d_noise, d_smooth))
    assert d_smooth <= 1 < d_noise


# ---- the library's host path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,data", SMALL + LARGE, ids=_ids(SMALL + LARGE))
def test_host_parser_and_entropy_equal_the_restatement(hm, key, data):
    from hydra_mi import videoio
    _frame, coef, _bad, g = ref.reference(key, data)
    info = videoio.mjpeg_probe(data)
    assert (info["W"], info["H"], info["components"], info["hs"], info["vs"], info["ri"], info["mcus"]) == \
        (g["W"], g["H"], g["components"], g["hs"], g["vs"], g["ri"], g["n_mcu"])
    assert videoio.mjpeg_intervals(data).tolist() == [list(iv) for iv in g["intervals"]]
    dec = videoio.MjpegDecoder(g["W"], g["H"])                 # (nothing runs on the device before the first decode)
    try:
        got, bad = dec.entropy_host(data)
    finally:
        dec.close()
    assert bad == 0 and got.shape == coef.shape and np.array_equal(got, coef)


def test_create_and_tune_refusals(hm):
    from hydra_mi import videoio
    for W, H, run, word in ((0, 8, 1, "frame size"), (8, 32768, 1, "frame size"), (8, 8, 0, "max_run"), (8, 8, 65, "max_run")):
        with pytest.raises(RuntimeError, match=word):
            videoio.MjpegDecoder(W, H, run)
    dec = videoio.MjpegDecoder(8, 8)
    try:
        for name, value in (("pool", 0), ("pool", 17), ("entropy", 3), ("auto_intervals", -1), ("nothing", 1)):
            with pytest.raises(RuntimeError, match=name):
                dec.tune(name, value)
        dec.tune("pool", 16)
    finally:
        dec.close()
    with pytest.raises(ValueError, match="entropy"):
        videoio.MjpegDecoder(8, 8, entropy="gpu")


def _refusals():
    from PIL import Image
    import io
    grey = cases.pil_save(cases.image(24, 24, 1), quality=75, restart_marker_rows=1)          # three intervals
    colour = cases.pil_save(cases.image(24, 24, 3), quality=75, subsampling=0)
    out = [("SOF2", cases.pil_save(cases.image(24, 24, 1), quality=75, progressive=True), "SOF2")]
    dqt = [s for s in cases.segments(grey) if s[0] == 0xDB][0][1]
    out.append(("dqt16", grey[:dqt + 4] + bytes([grey[dqt + 4] | 0x10]) + grey[dqt + 5:], "16-bit DQT"))
    b = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 4), np.uint8), "CMYK").save(b, "JPEG")
    out.append(("four_components", b.getvalue(), "4 components"))
    sos = [s for s in cases.segments(grey) if s[0] == 0xDA][0]
    eoi = grey.rindex(b"\xff\xd9")
    out.append(("second_scan", grey[:eoi] + grey[sos[1]:sos[1] + sos[2]] + b"\x00" + grey[eoi:], "second scan"))
    sof = [s for s in cases.segments(colour) if s[0] == 0xC0][0][1]
    assert colour[sof + 11] == 0x11
    out.append(("sampling_4x1", colour[:sof + 11] + b"\x41" + colour[sof + 12:], "sampling factors 4x1"))
    rst1 = grey.index(b"\xff\xd1")
    out.append(("missing_rst", grey[:rst1] + grey[rst1 + 2:], "RST markers"))
    out.append(("rst_out_of_turn", grey[:rst1] + b"\xff\xd3" + grey[rst1 + 2:], "RST3.*where RST1 is due"))
    out.append(("rst_without_dri", cases.without(grey, 0xDD), "without DRI"))
    return out


@pytest.mark.parametrize("name,data,message", _refusals(), ids=[r[0] for r in _refusals()])
def test_refusals_name_the_cause(hm, name, data, message):
    from hydra_mi import videoio
    with pytest.raises(ref.Refused):
        ref.parse(data)
    with pytest.raises(RuntimeError, match=message):
        videoio.mjpeg_probe(data)
    dec = videoio.MjpegDecoder(24, 24)
    try:
        with pytest.raises(RuntimeError, match=message):
            dec.entropy_host(data)
    finally:
        dec.close()


def test_another_size_is_refused(hm):
    from hydra_mi import videoio
    data = mjpeg_ref.reference("edge_7x9_c1")[0]
    dec = videoio.MjpegDecoder(9, 7)
    try:
        with pytest.raises(RuntimeError, match="7x9 for a decoder of 9x7"):
            dec.entropy_host(data)
    finally:
        dec.close()


# ---- bad intervals ---------------------------------------------------------------------------------------------------------
def test_bad_intervals_host_equals_restatement(hm):
    from hydra_mi import videoio
    clean, streams = cases.malformed()
    c_clean, bad, g = ref.coefficients(clean)
    assert bad == [] and len(g["intervals"]) == 4
    dec = videoio.MjpegDecoder(32, 32)
    try:
        for name, data in streams:
            want, bad, _ = ref.coefficients(data)
            got, count = dec.entropy_host(data)
            assert bad == [1] and count == 1, (name, bad, count)
            assert np.array_equal(got, want), name
            assert np.array_equal(got[:4], c_clean[:4]) and np.array_equal(got[8:], c_clean[8:]), name   # the others: untouched
            zero = np.flatnonzero(~got[4:8].any(axis=1))
            assert len(zero) >= 1 and zero[-1] == 3 and np.array_equal(zero, np.arange(zero[0], 4)), (name, zero)
            print("%s: blocks %d..3 of interval 1 are zero" % (name, zero[0]))
    finally:
        dec.close()


# ---- AviReader ---------------------------------------------------------------------------------------------------------------
def test_avi_reader_on_this_librarys_files(hm, tmp_path):
    from hydra_mi import videoio
    from hydra_mi.pipeline import load_video, to_gray
    frames = [cases.image(13, 7, 3) + k for k in range(3)]
    raw = str(tmp_path / "raw.avi")
    with videoio.AviWriter(raw, 13, 7, fps=20) as w:
        for f in frames:
            w.write(f)
    back = videoio.read_avi(raw)
    with videoio.AviReader(raw) as r:
        assert len(r) == 3 and r.shape == (7, 13) and r.fps == 20 and not r.mjpeg
        for k in range(3):
            assert np.array_equal(r.frame_bgr(k), back[k]) and np.array_equal(back[k], frames[k])
    assert np.array_equal(load_video(raw), to_gray(np.stack(frames)))            # (host path: no GPU)
    assert np.array_equal(load_video(raw, gray=False), np.stack(frames))
    grey = [cases.image(13, 7, 1) + k for k in range(3)]
    files = [mjpeg_ref.encode(f, 90, 1)[0] for f in grey]
    mj = str(tmp_path / "mj.avi")
    with videoio.AviWriter(mj, 13, 7, codec="mjpeg", channels=1) as w:
        for data in files:
            w.write_chunk(data)
    back = videoio.read_avi(mj)
    with videoio.AviReader(mj) as r:
        assert len(r) == 3 and r.shape == (7, 13) and r.mjpeg
        for k in range(3):
            assert bytes(r.chunk(k)) == files[k]
            assert np.array_equal(ref.decode(r.chunk(k))[0], back[k])
        with pytest.raises(ValueError, match="Motion-JPEG"):
            r.frame_bgr(0)


def test_avi_reader_on_a_foreign_container(hm, tmp_path):
    from hydra_mi import videoio
    from hydra_mi.pipeline import load_video, to_gray
    frames = [cases.image(5, 3, 3) + 7 * k for k in range(4)]
    data, want = cases.foreign_avi(frames)
    path = str(tmp_path / "foreign.avi")
    with open(path, "wb") as f:
        f.write(data)
    with videoio.AviReader(path) as r:
        assert len(r) == 4 and r.shape == (3, 5) and r.fps == 25 and r.top_down and not r.mjpeg
        for k in range(4):
            assert np.array_equal(r.frame_bgr(k), want[k]), k
    assert np.array_equal(load_video(path), to_gray(np.stack(want)))


@pytest.mark.parametrize("strf,message", [(cases.bitmapinfo(8, 8, 24, b"H264"), "H264"),
                                          (cases.bitmapinfo(8, 8, 8, 0) + b"\0" * 1024, "8-bit palettised")],
                         ids=["fourcc", "palettised"])
def test_avi_reader_refuses_by_name(hm, tmp_path, strf, message):
    from hydra_mi import videoio
    path = str(tmp_path / "x.avi")
    with open(path, "wb") as f:
        f.write(cases.tiny_avi(strf))
    with pytest.raises(ValueError, match=message):
        videoio.AviReader(path)
    with open(path, "wb") as f:
        f.write(b"RIFF\0\0\0\0WAVE")
    with pytest.raises(ValueError, match="not an AVI"):
        videoio.AviReader(path)


# ---- the shared routine keeps its bounds: a stand-alone program under the sanitizers ---------------------------------------------
def test_parser_and_entropy_routine_under_the_sanitizers(tmp_path):
    """built twice: at -O1, and at -O3 as the library is, so that what the optimiser makes of the routine is checked too"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    version = subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
    static = ["-static-libsan"] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    csrc = os.path.join(ROOT, "kalman-hydra_amd", "csrc")
    exes = []
    for opt in ("-O1", "-O3"):
        exes.append(str(tmp_path / ("mjpeg_dec_check" + opt)))
        subprocess.run([cxx, "-std=c++17", opt, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static +
                       ["-I", csrc, os.path.join(ROOT, "tools", "mjpeg_dec_check.cpp"), os.path.join(csrc, "mjpeg_dec.cpp"),
                        "-o", exes[-1], "-lpthread"], check=True)
    paths = []
    for name, data in (("grey_7x9.jpg", mjpeg_ref.reference("edge_7x9_c1")[0]),
                       ("c420_17x17.jpg", cases.pil_save(cases.image(17, 17, 3), quality=90, subsampling=2,
                                                         restart_marker_blocks=3))):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            f.write(data)
    for exe in exes:
        r = subprocess.run([exe] + paths, capture_output=True, text=True)
        print(r.stdout)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert r.stdout.count("inputs:") == 2

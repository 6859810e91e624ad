"""CPU checks of the Motion-JPEG path: the header the library builds against the restatement (tests/mjpeg_ref.py), the
restatement's streams through PIL's decoder (tables, size, mode), its integer DCT against a float64 one within the bound
DESIGN section 21 derives, its quality against PIL's own encoder, the symbols the GPU test's cases reach, the MJPG AVI
container read back chunk by chunk, and every refusal of hm_mjpeg_create / hm_avi_open_codec / hm_avi_write_chunk."""
import ctypes
import io
import math
import os
import struct

import numpy as np
import pytest

import mjpeg_ref


def _open(data):
    from PIL import Image
    img = Image.open(io.BytesIO(data))
    img.load()
    return img


def _segments(data):
    """[(marker, body)] of a JPEG file up to and including SOS"""
    out, p = [], 2
    assert data[:2] == b"\xff\xd8"
    while True:
        assert data[p] == 0xFF
        m, n = data[p + 1], int.from_bytes(data[p + 2:p + 4], "big")
        out.append((m, data[p + 4:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out


# ---- headers and decoding --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,ch,q,rr", [(61, 45, 3, 90, 1), (61, 45, 1, 90, 1), (1, 1, 3, 1, 1), (24, 80, 3, 49, 3),
                                         (2056, 16, 1, 100, 2), (32767, 8, 1, 50, 7), (640, 480, 3, 75, 4)])
def test_header_equals_the_restatement(hm, W, H, ch, q, rr):
    from hydra_mi.videoio import MjpegEncoder
    enc = MjpegEncoder(W, H, ch, q, rr)             # (nothing runs on the device before the first encode)
    try:
        assert enc.header == mjpeg_ref.header(W, H, ch, q, rr)
        blocks = ((W + 7) // 8) * ((H + 7) // 8) * ch
        intervals = -(-((H + 7) // 8) // rr)
        assert enc.max_bytes == len(enc.header) + 416 * blocks + 2 * intervals
    finally:
        enc.close()


@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("q", [1, 37, 50, 90, 100])
def test_pil_decodes_the_restatement_with_the_intended_tables(ch, q):
    frame = mjpeg_ref.smooth_image(37, 21, ch)
    data, _ = mjpeg_ref.encode(frame, q, 2)
    img = _open(data)
    assert img.size == (37, 21) and img.mode == ("RGB" if ch == 3 else "L")
    want = mjpeg_ref.quant_tables(q)
    # PIL reports the tables in natural order: a DQT written in natural instead of zigzag order would come back permuted
    assert {k: list(v) for k, v in img.quantization.items()} == {s: want[s] for s in range(2 if ch == 3 else 1)}
    if q == 100:
        assert all(v == 1 for tab in want for v in tab)


def test_huffman_tables_are_the_ones_libjpeg_writes():
    """the DHT segments of the restatement (and, by test_header_equals_the_restatement, of the library) hold the same
    BITS and HUFFVAL as the files of PIL's libjpeg, which uses the Annex K tables unless told to optimise"""
    from PIL import Image
    frame = mjpeg_ref.smooth_image(16, 16, 3)
    buf = io.BytesIO()
    Image.fromarray(frame).save(buf, "JPEG", quality=90, subsampling=0)

    def tables(data):
        out = {}
        for m, body in _segments(data):
            p = 0
            while m == 0xC4 and p < len(body):
                n = sum(body[p + 1:p + 17])
                out[body[p]] = body[p + 1:p + 17 + n]
                p += 17 + n
        return out
    ours = tables(mjpeg_ref.encode(frame, 90)[0])
    assert sorted(ours) == [0x00, 0x01, 0x10, 0x11] and ours == tables(buf.getvalue())


# ---- the DCT -----------------------------------------------------------------------------------------------------------
def _float_dct(block):
    c = np.array([[(math.sqrt(0.5) if u == 0 else 1.0) / 2 * math.cos((2 * x + 1) * u * math.pi / 16) for x in range(8)]
                  for u in range(8)])
    return c @ np.asarray(block, np.float64) @ c.T           # [v][u]


def test_dct_stays_within_the_derived_bound():
    E = mjpeg_ref.dct_bound()
    assert 0.6 < E < 0.7, E                                    # 0.66
    rng = np.random.default_rng(0)
    blocks = [rng.integers(-128, 128, (8, 8)) for _ in range(200)]
    blocks += [np.full((8, 8), v) for v in (-128, 127, 0)]
    yy, xx = np.mgrid[0:8, 0:8]
    blocks += [np.where((xx + yy) & 1, 127, -128), np.where((xx + yy) & 1, -128, 127), np.where(xx & 1, 127, -128),
               np.where(yy < 4, -128, 127), np.where(xx < 4, 127, -128)]
    for u in range(8):                                         # single basis functions at full swing, both signs
        for v in range(8):
            b = np.outer(np.cos((2 * np.arange(8) + 1) * v * np.pi / 16), np.cos((2 * np.arange(8) + 1) * u * np.pi / 16))
            blocks += [np.where(b > 0, 127, -128), np.where(b > 0, -128, 127), np.rint(127 * b).astype(int)]
    worst = 0.0
    for b in blocks:
        fixed = np.array(mjpeg_ref.fdct([[int(v) for v in row] for row in b]), np.float64) / mjpeg_ref.COEF_ONE
        assert np.abs(fixed).max() < 1024.5                     # a DC difference within category 11 at quality 100
        assert np.abs(fixed[np.arange(64).reshape(8, 8) > 0]).max() < 1023.5       # and no AC past size 10
        worst = max(worst, np.abs(fixed - _float_dct(b)).max())
    print("largest |fixed - float64| %.4f, bound %.4f" % (worst, E))
    assert worst <= E


# ---- quality against PIL's encoder ---------------------------------------------------------------------------------------
def _psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return 10 * np.log10(255.0 ** 2 / max(np.mean(d * d), 1e-12))


def _decode(data):
    img = _open(data)
    return np.asarray(img) if img.mode == "L" else np.asarray(img.convert("RGB"))[:, :, ::-1]


def _pil_encode(frame, q):
    from PIL import Image
    tabs = mjpeg_ref.quant_tables(q)
    buf = io.BytesIO()
    if frame.ndim == 2:
        Image.fromarray(frame).save(buf, "JPEG", qtables=[tabs[0]], restart_marker_rows=1)
    else:
        Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(buf, "JPEG", qtables=tabs, subsampling=0,
                                                                      restart_marker_rows=1)
    return buf.getvalue()


def _quality_images():
    W, H = 61, 45
    smooth = mjpeg_ref.smooth_image(W, H, 3)
    rng = np.random.default_rng(11)
    noisy = np.clip(smooth.astype(np.int16) + rng.integers(-20, 21, smooth.shape), 0, 255).astype(np.uint8)
    return {"smooth": smooth, "smooth_noise20": noisy, "noise": rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
            "grey": mjpeg_ref.smooth_image(W, H, 1)}


_quality_cache = {}


def _pil_psnr(image, frame, q):
    """PSNR and size of PIL's own coding at quality q, computed once per (image, q)"""
    if (image, q) not in _quality_cache:
        data = _pil_encode(frame, q)
        _quality_cache[image, q] = (_psnr(_decode(data), frame), len(data), data)
    return _quality_cache[image, q]


@pytest.mark.parametrize("q", [50, 75, 90, 100])
@pytest.mark.parametrize("image", ["smooth", "smooth_noise20", "noise", "grey"])
def test_quality_is_within_a_quarter_step_of_pil(image, q):
    """ours(q) >= PIL(q) - (PIL(q) - PIL(q - 5)) / 4: PIL with the same tables, no subsampling and a restart marker per
    row of blocks, both decoded by PIL.

    The coefficient goes to the quantiser in eighths, as libjpeg's does.  Quantising a coefficient already rounded to an
    integer loses up to 0.025 dB on smooth_noise20, whose per-channel noise the chroma tables remove at every quality up
    to 75, so that PIL's own step from 70 to 75 is 0.08 dB there and the bound a fiftieth of a dB: that version missed
    [smooth_noise20-75] by 0.0227 against 0.0204 dB.  Now the tightest case is that one at 0.0076 of 0.0204 dB (the table
    is in DESIGN section 21)."""
    frame = _quality_images()[image]
    ours_data, _ = mjpeg_ref.encode(frame, q, 1)
    (pil, pil_bytes, pil_data), (low, _, _) = _pil_psnr(image, frame, q), _pil_psnr(image, frame, q - 5)
    assert {k: list(v) for k, v in _open(pil_data).quantization.items()} == \
        {k: list(v) for k, v in _open(ours_data).quantization.items()}                   # the same tables indeed
    ours = _psnr(_decode(ours_data), frame)
    print("%-15s q %3d: ours %.3f dB, PIL %.3f dB, PIL(q-5) %.3f dB, deficit %.4f of %.4f; bytes %d against %d"
          % (image, q, ours, pil, low, pil - ours, 0.25 * (pil - low), len(ours_data), pil_bytes))
    assert pil - low > 0
    assert pil - ours <= 0.25 * (pil - low), (image, q, ours, pil, low)


# ---- what the GPU test's cases reach ---------------------------------------------------------------------------------------
def test_cases_cover_the_hard_symbols():
    seen, most_intervals = {}, 0
    for name, frame, q, rr in mjpeg_ref.cases():
        data, hist = mjpeg_ref.reference(name)
        img = _open(data)
        assert img.size == (frame.shape[1], frame.shape[0]), name
        for k, v in hist.items():
            seen[k] = seen.get(k, 0) + v
        most_intervals = max(most_intervals, hist["intervals"])
    for key in ("dc0", "dc11", "ac10", "zrl", "no_eob", "eob", "stuffed"):
        assert seen.get(key, 0) > 0, key
    assert most_intervals > 8
    names = [c[0] for c in mjpeg_ref.cases()]
    assert len(set(names)) == len(names)


# ---- the container --------------------------------------------------------------------------------------------------------
def _chunks(b, start, end):
    out, p = [], start
    while p + 8 <= end:
        cc, size = b[p:p + 4], struct.unpack_from("<I", b, p + 4)[0]
        if cc in (b"RIFF", b"LIST"):
            out.append((b[p + 8:p + 12], p + 12, size - 4))
        else:
            out.append((cc, p + 8, size))
        p += 8 + size + (size & 1)
    assert p == end
    return out


def _jpegs(n, W, H, ch):
    """n small JPEG files of odd and even lengths (a byte after EOI, which decoders ignore, makes the parity)"""
    out = []
    for k in range(n):
        f = np.roll(mjpeg_ref.smooth_image(W, H, ch), 3 * k, axis=1)
        d = mjpeg_ref.encode(f, 60 + 5 * (k % 4), 1)[0]
        if len(d) % 2 == k % 2:                     # even k: odd length
            d += b"\0"
        out.append(d)
    return out


@pytest.mark.parametrize("ch", [3, 1])
def test_mjpg_avi_headers_indexes_padding_and_continuation(hm, tmp_path, ch):
    from hydra_mi import _lib, videoio
    L = _lib.lib()
    W, H, n = 37, 21, 64
    data = _jpegs(n, W, H, ch)
    assert any(len(d) & 1 for d in data) and any(not len(d) & 1 for d in data)
    path = str(tmp_path / "m.avi")
    limit = 16384                                   # the least: the headers take 4.7 KB of the first RIFF
    h = _lib.c_vp()
    _lib.check(L.hm_avi_open_codec(path.encode(), W, H, 20, limit, 1, ctypes.byref(h)), "hm_avi_open_codec")
    for d in data:
        buf = np.frombuffer(d, np.uint8)
        _lib.check(L.hm_avi_write_chunk(h, _lib.ptr(buf), len(d)), "hm_avi_write_chunk")
    _lib.check(L.hm_avi_close(h), "hm_avi_close")
    b = open(path, "rb").read()
    riffs = _chunks(b, 0, len(b))
    assert len(riffs) >= 3 and riffs[0][0] == b"AVI " and all(r[0] == b"AVIX" for r in riffs[1:])
    assert all(8 + 4 + r[2] <= limit for r in riffs)                      # decided by the bytes actually written
    top = {c[0]: c for c in _chunks(b, riffs[0][1], riffs[0][1] + riffs[0][2])}
    hdrl = {c[0]: c for c in _chunks(b, top[b"hdrl"][1], top[b"hdrl"][1] + top[b"hdrl"][2])}
    strl = {c[0]: c for c in _chunks(b, hdrl[b"strl"][1], hdrl[b"strl"][1] + hdrl[b"strl"][2])}
    avih = struct.unpack_from("<10I", b, hdrl[b"avih"][1])
    strh = b[strl[b"strh"][1]:strl[b"strh"][1] + 56]
    bih = struct.unpack_from("<IiiHH4sI", b, strl[b"strf"][1])
    largest = max(len(d) for d in data)
    assert avih[0] == 50000 and avih[1] == largest * 20 and avih[7] == largest + 8 and (avih[8], avih[9]) == (W, H)
    assert strh[0:4] == b"vids" and strh[4:8] == b"MJPG"
    assert struct.unpack_from("<I", strh, 32)[0] == n                     # dwLength
    assert struct.unpack_from("<I", strh, 36)[0] == largest + 8           # dwSuggestedBufferSize
    assert struct.unpack_from("<I", strh, 44)[0] == 0                     # dwSampleSize
    assert bih[:6] == (40, W, H, 1, 24, b"MJPG")
    odml = _chunks(b, hdrl[b"odml"][1], hdrl[b"odml"][1] + hdrl[b"odml"][2])
    assert struct.unpack_from("<I", b, odml[0][1])[0] == n
    # idx1: the first RIFF's chunks, each with its own size and the key-frame flag
    movi0, idx1 = top[b"movi"], top[b"idx1"]
    n1 = idx1[2] // 16
    assert avih[4] == n1 and 0 < n1 < n
    for i in range(n1):
        ck, flags, off, size = struct.unpack_from("<4sIII", b, idx1[1] + 16 * i)
        p = movi0[1] - 4 + off
        assert ck == b"00dc" and flags == 0x10 and size == len(data[i])
        assert b[p:p + 4] == b"00dc" and b[p + 8:p + 8 + size] == data[i]
    # indx -> ix00 -> every chunk, with its own size; odd chunks are followed by one zero byte
    indx = strl[b"indx"]
    wl, sub, typ, used, cid = struct.unpack_from("<HBBI4s", b, indx[1])
    assert (wl, sub, typ, cid) == (4, 0, 0, b"00dc") and used == len(riffs)
    got = []
    for e in range(used):
        off, size, dur = struct.unpack_from("<QII", b, indx[1] + 24 + 16 * e)
        assert b[off:off + 4] == b"ix00" and struct.unpack_from("<I", b, off + 4)[0] + 8 == size
        wl2, sub2, typ2, k, cid2, base = struct.unpack_from("<HBBI4sQ", b, off + 8)
        assert (wl2, sub2, typ2, cid2) == (2, 0, 1, b"00dc") and k == dur
        for i in range(k):
            o, s = struct.unpack_from("<II", b, off + 32 + 8 * i)
            assert b[base + o - 8:base + o - 4] == b"00dc" and struct.unpack_from("<I", b, base + o - 4)[0] == s
            if s & 1:
                assert b[base + o + s] == 0
            got.append(b[base + o:base + o + s])
    assert got == data
    # read_avi: what PIL decodes from each chunk
    frames = videoio.read_avi(path)
    assert len(frames) == n
    for f, d in zip(frames, data):
        assert f.shape == ((H, W, 3) if ch == 3 else (H, W)) and np.array_equal(f, _decode(d))


def _assemble_raw_avi(frames, W, H, fps, limit):
    """The bytes of the library's uncompressed AVI, put together here from the layout tests/test_views_cpu.py reads back
    and the rules of include/hydra_mi.h: hdrl (avih, strl with strh, strf and a 256-entry 'indx', odml/dmlh), then per RIFF
    a 'movi' of '00db' chunks (rows bottom-up, padded to 4 bytes) closed by its 'ix00', 'idx1' after the first; a frame that
    would take the RIFF, its 'ix00' and (first RIFF) 'idx1' past `limit` opens the next 'AVIX'."""
    u16, u32, u64 = (lambda v: struct.pack("<H", v)), (lambda v: struct.pack("<I", v)), (lambda v: struct.pack("<Q", v))
    stride = (3 * W + 3) & ~3
    fb = stride * H
    idx_bytes = 24 + 16 * 256
    strl = 4 + (8 + 56) + (8 + 40) + (8 + idx_bytes)
    odml = 4 + 8 + 248
    out = bytearray()
    out += b"RIFF" + u32(0) + b"AVI "
    out += b"LIST" + u32(4 + (8 + 56) + (8 + strl) + (8 + odml)) + b"hdrl"
    out += b"avih" + u32(56) + u32(1000000 // fps) + u32(fb * fps) + u32(0) + u32(0x10)
    avih_frames = len(out)
    out += u32(0) + u32(0) + u32(1) + u32(fb + 8) + u32(W) + u32(H) + u32(0) * 4
    out += b"LIST" + u32(strl) + b"strl"
    out += b"strh" + u32(56) + b"vids" + b"DIB " + u32(0) + u16(0) + u16(0) + u32(0) + u32(1) + u32(fps) + u32(0)
    strh_length = len(out)
    out += u32(0) + u32(fb + 8) + u32(0xFFFFFFFF) + u32(fb) + u16(0) + u16(0) + u16(W) + u16(H)
    out += b"strf" + u32(40) + u32(40) + u32(W) + u32(H) + u16(1) + u16(24) + u32(0) + u32(fb) + u32(0) * 4
    indx = len(out)
    out += b"indx" + u32(idx_bytes) + u16(4) + b"\0\0" + u32(0) + b"00db" + u32(0) * 3 + bytes(16 * 256)
    out += b"LIST" + u32(odml) + b"odml" + b"dmlh" + u32(248)
    dmlh = len(out)
    out += bytes(248)
    riff_pos, first, supers = 0, True, []
    movi = len(out)
    out += b"LIST" + u32(0) + b"movi"
    chunks = []

    def close_riff():
        k = len(chunks)
        supers.append((len(out), 32 + 8 * k, k))
        out.extend(b"ix00" + u32(24 + 8 * k) + u16(2) + b"\0\1" + u32(k) + b"00db" + u64(movi) + u32(0))
        for c in chunks:
            out.extend(u32(c + 8 - movi) + u32(fb))
        out[movi + 4:movi + 8] = u32(len(out) - movi - 8)
        if first:
            out[avih_frames:avih_frames + 4] = u32(k)
            out.extend(b"idx1" + u32(16 * k))
            for c in chunks:
                out.extend(b"00db" + u32(0x10) + u32(c - (movi + 8)) + u32(fb))
        out[riff_pos + 4:riff_pos + 8] = u32(len(out) - riff_pos - 8)

    for f in frames:
        k = len(chunks)
        need = len(out) + 8 + fb + 32 + 8 * (k + 1) + (8 + 16 * (k + 1) if first else 0) - riff_pos
        if k > 0 and need > limit:
            close_riff()
            first = False
            riff_pos = len(out)
            out += b"RIFF" + u32(0) + b"AVIX"
            movi = len(out)
            out += b"LIST" + u32(0) + b"movi"
            chunks = []
        chunks.append(len(out))
        out += b"00db" + u32(fb)
        for r in range(H - 1, -1, -1):
            out += f[r].tobytes() + bytes(stride - 3 * W)
    close_riff()
    n = len(frames)
    out[strh_length:strh_length + 4] = u32(n)
    out[dmlh:dmlh + 4] = u32(n)
    out[indx + 12:indx + 16] = u32(len(supers))
    for i, (off, size, dur) in enumerate(supers):
        out[indx + 32 + 16 * i:indx + 48 + 16 * i] = u64(off) + u32(size) + u32(dur)
    return bytes(out)


def test_raw_avi_is_byte_identical(hm, tmp_path):
    """a raw AVI of this build, through hm_avi_open, through hm_avi_open_codec(HM_AVI_RAW) and through AviWriter, is byte
    for byte the file _assemble_raw_avi puts together from the rules (two RIFFs, rows with a byte of padding), passes the
    reader of tests/test_views_cpu.py, and read_avi gives the frames back"""
    from hydra_mi import _lib, videoio
    from test_views_cpu import read_avi
    L = _lib.lib()
    W, H, n = 5, 3, 200
    frames = np.random.default_rng(5).integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    limit = 2 * (16 * 3 + 8) + 16384                 # the least the library takes: 147 frames fit the first RIFF
    want = _assemble_raw_avi(frames, W, H, 20, limit)
    for how in ("open", "open_codec", "writer"):
        path = str(tmp_path / (how + ".avi"))
        if how == "writer":
            with videoio.AviWriter(path, W, H, riff_limit=limit) as v:
                for f in frames:
                    v.write(f)
        else:
            h = _lib.c_vp()
            if how == "open":
                _lib.check(L.hm_avi_open(path.encode(), W, H, 20, limit, ctypes.byref(h)), "hm_avi_open")
            else:
                _lib.check(L.hm_avi_open_codec(path.encode(), W, H, 20, limit, 0, ctypes.byref(h)), "hm_avi_open_codec")
            for f in frames:
                _lib.check(L.hm_avi_write(h, _lib.ptr(np.ascontiguousarray(f))), "hm_avi_write")
            _lib.check(L.hm_avi_close(h), "hm_avi_close")
        got = open(path, "rb").read()
        assert len(got) == len(want), how
        assert got == want, (how, next(i for i in range(len(want)) if got[i] != want[i]))
    info = read_avi(path)
    assert info["riffs"] == 2 and info["total"] == n and info["handler"] == b"DIB "
    back = videoio.read_avi(path)
    assert len(back) == n and all(np.array_equal(a, f) for a, f in zip(back, frames))


def test_grey_frames_into_a_raw_video(hm, tmp_path):
    from hydra_mi import videoio
    plane = mjpeg_ref.smooth_image(9, 6, 1)
    path = str(tmp_path / "g.avi")
    with videoio.AviWriter(path, 9, 6, channels=1) as v:
        v.write(plane)
        v.write_grey(plane)
        v.write(np.repeat(plane[:, :, None], 3, axis=2))
    back = videoio.read_avi(path)
    assert len(back) == 3 and all(np.array_equal(f, np.repeat(plane[:, :, None], 3, axis=2)) for f in back)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,match", [
    ((0, 8, 3, 90, 1), r"frame size 0x8 outside 1\.\.32767"),
    ((8, 32768, 3, 90, 1), r"frame size 8x32768 outside 1\.\.32767"),
    ((8, 8, 2, 90, 1), r"2 channels, not 1 or 3"),
    ((8, 8, 3, 0, 1), r"quality 0 outside 1\.\.100"),
    ((8, 8, 3, 101, 1), r"quality 101 outside 1\.\.100"),
    ((8, 8, 3, 90, 0), r"restart_rows 0 below 1"),
    ((32767, 128, 1, 90, 16), r"65536 blocks in a restart interval \(4096 across, 16 rows\), more than 65535"),
    ((32767, 32767, 3, 90, 1), r"can code to \d+ bytes, 2\^31 or more"),
])
def test_create_refusals_name_the_numbers(hm, args, match):
    from hydra_mi import _lib
    h = _lib.c_vp()
    rc = _lib.lib().hm_mjpeg_create(0, *args, ctypes.byref(h))
    assert rc != 0 and h.value is None
    with pytest.raises(RuntimeError, match=match):
        _lib.check(rc, "hm_mjpeg_create")


def test_other_refusals(hm, tmp_path):
    from hydra_mi import _lib, videoio
    L = _lib.lib()
    enc = videoio.MjpegEncoder(16, 16, 3, 90, 1)
    n = ctypes.c_uint64()
    buf = np.empty(len(enc.header) - 1, np.uint8)
    with pytest.raises(RuntimeError, match="the header has %d bytes, the buffer %d" % (len(enc.header), buf.nbytes)):
        _lib.check(L.hm_mjpeg_header(enc._h, _lib.ptr(buf), buf.nbytes, ctypes.byref(n)), "hm_mjpeg_header")
    with pytest.raises(ValueError, match="frame of shape"):
        enc.encode(np.zeros((16, 16), np.uint8))
    enc.close()
    h = _lib.c_vp()
    with pytest.raises(RuntimeError, match="codec 7"):
        _lib.check(L.hm_avi_open_codec(str(tmp_path / "a.avi").encode(), 8, 8, 20, 0, 7, ctypes.byref(h)), "open")
    with pytest.raises(RuntimeError, match="RIFF limit of 1000 bytes"):
        _lib.check(L.hm_avi_open_codec(str(tmp_path / "a.avi").encode(), 8, 8, 20, 1000, 1, ctypes.byref(h)), "open")
    one = np.zeros(4, np.uint8)
    _lib.check(L.hm_avi_open_codec(str(tmp_path / "a.avi").encode(), 8, 8, 20, 0, 1, ctypes.byref(h)), "open")
    with pytest.raises(RuntimeError, match="opened for compressed chunks"):
        _lib.check(L.hm_avi_write(h, _lib.ptr(np.zeros((8, 8, 3), np.uint8))), "hm_avi_write")
    with pytest.raises(RuntimeError, match="a chunk of 0 bytes"):
        _lib.check(L.hm_avi_write_chunk(h, _lib.ptr(one), 0), "hm_avi_write_chunk")
    _lib.check(L.hm_avi_close(h), "hm_avi_close")
    _lib.check(L.hm_avi_open(str(tmp_path / "b.avi").encode(), 8, 8, 20, 0, ctypes.byref(h)), "open")
    with pytest.raises(RuntimeError, match="opened for uncompressed frames"):
        _lib.check(L.hm_avi_write_chunk(h, _lib.ptr(one), 4), "hm_avi_write_chunk")
    _lib.check(L.hm_avi_close(h), "hm_avi_close")
    with pytest.raises(ValueError, match="codec 'h264'"):
        videoio.AviWriter(str(tmp_path / "c.avi"), 8, 8, codec="h264")
    with videoio.AviWriter(str(tmp_path / "d.avi"), 8, 8) as v:
        with pytest.raises(ValueError, match="not MJPEG"):
            v.write_dev(0, None)


def test_cli_passes_the_codec_to_every_writer(hm, monkeypatch, tmp_path):
    """--video-codec mjpeg --video-quality reach the overlay writer (three components) and --registered (one); without the
    flag the writers are called as they always were"""
    import sys
    from test_views_cpu import _StubKF, _cli
    cli = _cli(monkeypatch, tmp_path)
    made = []

    class _W:
        def __init__(self, *a, **k):
            made.append((a, k))
            self.frames = 0

        def write(self, img):
            self.frames += 1

        def close(self):
            pass

    class _R:
        def view(self, X, which):
            return np.zeros((8, 8, 3), np.uint8)

    def compute(self, *a, **kw):
        self.state.renderer = _R()
        return (0, 0.0, 0.0, 0, None, None)
    monkeypatch.setattr(cli, "AviWriter", _W)
    monkeypatch.setattr(_StubKF, "compute", compute)
    assert cli.main(["in.npy", "flow", "out.avi", "--video-codec", "mjpeg", "--video-quality", "77"]) == 0
    assert made == [(("out.avi", 8, 8), dict(codec="mjpeg", quality=77))]
    del made[:]
    assert cli.main(["in.npy", "flow", "out.avi"]) == 0
    assert made == [(("out.avi", 8, 8), {})]
    with pytest.raises(SystemExit):
        cli.main(["in.npy", "flow", "out.avi", "--video-codec", "mjpeg", "--video-quality", "0"])
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import optical_flow_ext as tool
    assert tool._video_opts(["x", "--video-codec", "mjpeg", "v.npy", "--video-quality", "60", "f"]) == \
        (["x", "v.npy", "f"], dict(codec="mjpeg", quality=60))
    assert tool._video_opts(["x", "v.npy", "f"]) == (["x", "v.npy", "f"], {})
    assert tool._video_opts(["x", "--video-codec", "gif"])[1] is None and tool._video_opts(["--video-quality"])[1] is None

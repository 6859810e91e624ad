"""The Motion-JPEG decoder of include/hydra_mi.h ("Motion-JPEG, decoding") restated in loops and Python integers, from the
rules written there and not from the library: ``parse`` gives a file's geometry, tables and interval table or raises
``Refused``; ``coefficients`` the zigzag coefficients of every luma block and the bad intervals; ``decode`` the grey frame.
The library must give these numbers.  Slow on purpose (a 61x45 frame takes a fraction of a second)."""
import numpy as np

import mjpeg_ref

ZIGZAG = mjpeg_ref.ZIGZAG
M32 = 0xFFFFFFFF


class Refused(ValueError):
    pass


def _codes(bits, vals):
    """(length, code) -> symbol, the canonical codes of T.81 Annex C"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            if code >= 1 << length:
                raise Refused("DHT: more codes of a length than exist")
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


def annex_k(cls, idx):
    if idx > 1:
        raise Refused("Huffman table class %d index %d is not defined" % (cls, idx))
    if cls == 0:
        return _codes(mjpeg_ref.DC_BITS[idx], mjpeg_ref.DC_VALS)
    return _codes(mjpeg_ref.AC_BITS[idx], mjpeg_ref.AC_VALS[idx])


def parse(b):
    """-> dict(W, H, components, hs, vs, ri, quant (luma, zigzag order), tables [(dc, ac)] per component, mw, mh, n_mcu,
    per (MCUs of an interval), intervals [(start, end, first_mcu)])"""
    b = bytes(b)
    n = len(b)
    if n < 4 or b[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    quant, huff, comps, ri, sof = {}, {}, [], 0, None
    p = 2
    while True:
        if p + 2 > n:
            raise Refused("the file ends before SOS")
        if b[p] != 0xFF:
            raise Refused("no marker at %d" % p)
        if b[p + 1] == 0xFF:
            p += 1
            continue
        m = b[p + 1]
        p += 2
        if m == 0xD9:
            raise Refused("EOI before SOS")
        if m in (0x00, 0x01, 0xD8) or 0xD0 <= m <= 0xD7:
            raise Refused("marker FF%02X before SOS" % m)
        if p + 2 > n:
            raise Refused("the file ends inside a marker")
        L = int.from_bytes(b[p:p + 2], "big")
        if L < 2 or p + L > n:
            raise Refused("segment FF%02X does not fit" % m)
        s = b[p + 2:p + L]
        if m == 0xC0:
            if sof is not None or len(s) < 6:
                raise Refused("SOF0")
            if s[0] != 8:
                raise Refused("sample precision %d" % s[0])
            H, W, N = int.from_bytes(s[1:3], "big"), int.from_bytes(s[3:5], "big"), s[5]
            if W < 1 or H < 1:
                raise Refused("frame size")
            if N not in (1, 3):
                raise Refused("%d components" % N)
            if len(s) != 6 + 3 * N:
                raise Refused("SOF0 length")
            for c in range(N):
                cid, hv, tq = s[6 + 3 * c], s[7 + 3 * c], s[8 + 3 * c]
                h, v = hv >> 4, hv & 15
                ok = (1 <= h <= 4 and 1 <= v <= 4) if N == 1 else (h in (1, 2) and v in (1, 2)) if c == 0 else (h, v) == (1, 1)
                if not ok:
                    raise Refused("sampling factors %dx%d" % (h, v))
                if tq > 3:
                    raise Refused("quantisation table %d" % tq)
                comps.append((cid, h, v, tq))
            sof = (W, H, N)
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Refused("SOF%d" % (m - 0xC0))
        elif m == 0xCC:
            raise Refused("DAC: arithmetic coding")
        elif m == 0xC8:
            raise Refused("JPG extension")
        elif m == 0xC4:
            i = 0
            while i < len(s):
                if i + 17 > len(s):
                    raise Refused("DHT ends inside a table")
                tc, th = s[i] >> 4, s[i] & 15
                if tc > 1 or th > 3:
                    raise Refused("DHT class %d index %d" % (tc, th))
                bits = list(s[i + 1:i + 17])
                nv = sum(bits)
                if nv > 256 or i + 17 + nv > len(s):
                    raise Refused("DHT does not fit")
                huff[(tc, th)] = _codes(bits, s[i + 17:i + 17 + nv])
                i += 17 + nv
        elif m == 0xDB:
            i = 0
            while i < len(s):
                pq, tq = s[i] >> 4, s[i] & 15
                if pq != 0:
                    raise Refused("16-bit DQT")
                if tq > 3 or i + 65 > len(s):
                    raise Refused("DQT does not fit")
                quant[tq] = list(s[i + 1:i + 65])
                i += 65
        elif m == 0xDD:
            if len(s) != 2:
                raise Refused("DRI length")
            ri = int.from_bytes(s, "big")
        elif m == 0xDA:
            if sof is None:
                raise Refused("SOS before SOF0")
            W, H, N = sof
            if len(s) < 1 or len(s) != 4 + 2 * s[0]:
                raise Refused("SOS length")
            if s[0] != N:
                raise Refused("a scan of %d of the %d components (several scans)" % (s[0], N))
            tables = []
            for c in range(N):
                cid, td, ta = s[1 + 2 * c], s[2 + 2 * c] >> 4, s[2 + 2 * c] & 15
                if cid != comps[c][0]:
                    raise Refused("SOS component")
                if td > 3 or ta > 3:
                    raise Refused("SOS tables")
                tables.append((huff[(0, td)] if (0, td) in huff else annex_k(0, td),
                               huff[(1, ta)] if (1, ta) in huff else annex_k(1, ta)))
            if tuple(s[1 + 2 * N:]) != (0, 63, 0):
                raise Refused("not a baseline scan")
            if comps[0][3] not in quant:
                raise Refused("quantisation table not defined")
            p += L
            break
        p += L
    hs, vs = (comps[0][1], comps[0][2]) if N == 3 else (1, 1)
    mw, mh = -(-W // (8 * hs)), -(-H // (8 * vs))
    n_mcu = mw * mh
    per = ri if ri else n_mcu
    expect = -(-n_mcu // per)
    intervals, start, i, eoi = [], p, p, False
    while i + 1 < n:
        if b[i] != 0xFF or b[i + 1] in (0x00, 0xFF):
            i += 1
            continue
        m = b[i + 1]
        if m == 0xD9:
            eoi = True
            break
        if m == 0xDA:
            raise Refused("a second scan")
        if not 0xD0 <= m <= 0xD7:
            raise Refused("marker FF%02X inside the scan" % m)
        if not ri:
            raise Refused("RST without DRI")
        k = len(intervals)
        if k + 1 >= expect:
            raise Refused("more RST markers than intervals")
        if m - 0xD0 != k & 7:
            raise Refused("RST%d where RST%d is due" % (m - 0xD0, k & 7))
        intervals.append((start, i, k * per))
        start = i = i + 2
    if len(intervals) + 1 != expect:
        raise Refused("%d RST markers, %d are needed" % (len(intervals), expect - 1))
    intervals.append((start, i if eoi else n, len(intervals) * per))
    return dict(W=W, H=H, components=N, hs=hs, vs=vs, ri=ri, quant=quant[comps[0][3]], tables=tables, mw=mw, mh=mh, n_mcu=n_mcu,
                per=per, intervals=intervals)


class _Bad(Exception):
    pass


class _Bits:
    """the bits of bytes [p, end): FF 00 is FF, an FF that no 00 follows ends the data"""

    def __init__(self, b, p, end):
        self.b, self.p, self.end, self.acc, self.n = b, p, end, 0, 0

    def bit(self):
        if self.n == 0:
            if self.p >= self.end:
                raise _Bad("the bytes ran out")
            v = self.b[self.p]
            if v == 0xFF:
                if self.end - self.p >= 2 and self.b[self.p + 1] == 0:
                    self.p += 2
                else:
                    self.p = self.end
                    raise _Bad("the bytes ran out")
            else:
                self.p += 1
            self.acc, self.n = v, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def value(self, k):
        v = 0
        for _ in range(k):
            v = 2 * v + self.bit()
        return v if k == 0 or v >= 1 << (k - 1) else v - (1 << k) + 1

    def symbol(self, tab):
        c = 0
        for length in range(1, 17):
            c = 2 * c + self.bit()
            if (length, c) in tab:
                return tab[(length, c)]
        raise _Bad("a code of no table")


def _wrap16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def _block(bs, dc, ac, pred, c, keep):
    t = bs.symbol(dc)
    if t > 11:
        raise _Bad("DC category %d" % t)
    pred[c] = (pred[c] + bs.value(t)) & M32
    zz = [0] * 64
    zz[0] = _wrap16(pred[c])
    k = 1
    while k < 64:
        rs = bs.symbol(ac)
        r, size = rs >> 4, rs & 15
        if size == 0:
            if r != 15:
                break
            k += 16
            if k > 63:
                raise _Bad("ZRL leaves the block")
            continue
        if size > 10:
            raise _Bad("AC size %d" % size)
        k += r
        if k > 63:
            raise _Bad("a run leaves the block")
        zz[k] = bs.value(size)
        k += 1
    return zz if keep else None


def coefficients(b, info=None):
    """-> (int16 array (luma blocks in scan order, 64) in zigzag order, [indices of bad intervals], info)"""
    b = bytes(b)
    g = info or parse(b)
    lb = g["hs"] * g["vs"]
    coef = np.zeros((g["n_mcu"] * lb, 64), np.int16)
    bad = []
    for idx, (start, end, first) in enumerate(g["intervals"]):
        bs = _Bits(b, start, end)
        pred = [0, 0, 0]
        ok = True
        for m in range(first, min(first + g["per"], g["n_mcu"])):
            if not ok:
                break                                             # (the rest of the interval stays zero)
            try:
                for j in range(lb):
                    at = m * lb + j
                    coef[at] = _block(bs, g["tables"][0][0], g["tables"][0][1], pred, 0, True)
                at = (m + 1) * lb                                 # (a bad chroma block: the MCU's luma blocks stay)
                for c in range(1, g["components"]):
                    _block(bs, g["tables"][c][0], g["tables"][c][1], pred, c, False)
            except _Bad:
                ok = False
                bad.append(idx)
                coef[at:(m + 1) * lb] = 0                         # the bad block; the later ones were never written
    return coef, bad, g


def _fix(x):
    return int(x * 8192 + 0.5)


_C = {k: _fix(v) for k, v in dict(a=0.298631336, b=0.390180644, c=0.541196100, d=0.765366865, e=0.899976223, f=1.175875602,
                                  g=1.501321110, h=1.847759065, i=1.961570560, j=2.053119869, k=2.562915447, l=3.072711026).items()}


def _signed(x):
    x &= M32
    return x - (1 << 32) if x & 0x80000000 else x


def _pass(d, shift):
    """one 8-point pass of jidctint.c; every sum is masked to 32 bits, the shift is of the signed value"""
    C = _C
    z1 = ((d[2] + d[6]) * C["c"]) & M32
    t2 = (z1 - d[6] * C["h"]) & M32
    t3 = (z1 + d[2] * C["d"]) & M32
    t0 = ((d[0] + d[4]) << 13) & M32
    t1 = ((d[0] - d[4]) << 13) & M32
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * C["f"]
    a0, a1, a2, a3 = a0 * C["a"], a1 * C["j"], a2 * C["l"], a3 * C["g"]
    z1, z2, z3, z4 = -z1 * C["e"], -z2 * C["k"], -z3 * C["i"] + z5, -z4 * C["b"] + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    r = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return [_signed(x + (1 << (shift - 1))) >> shift for x in r]      # (mod 2^32 arithmetic: masking once at the end is the same)


def _limit(x):
    x &= 1023
    return x + 128 if x < 128 else 255 if x < 512 else 0 if x < 896 else x - 896


def idct(zz, quant):
    """zigzag coefficients and table -> 8 rows of 8 samples"""
    co = [[0] * 8 for _ in range(8)]
    for k in range(64):
        co[ZIGZAG[k] // 8][ZIGZAG[k] % 8] = int(zz[k]) * quant[k]
    ws = [[0] * 8 for _ in range(8)]
    for u in range(8):
        col = _pass([co[v][u] for v in range(8)], 11)
        for v in range(8):
            ws[v][u] = col[v]
    return [[_limit(x) for x in _pass(ws[v], 18)] for v in range(8)]


def frame_of(coef, g):
    W, H, hs, vs, mw = g["W"], g["H"], g["hs"], g["vs"], g["mw"]
    lb = hs * vs
    out = np.zeros((g["mh"] * vs * 8, mw * hs * 8), np.uint8)
    cache = {}
    for b in range(coef.shape[0]):
        key = coef[b].tobytes()
        if key not in cache:
            cache[key] = np.array(idct(coef[b], g["quant"]), np.uint8)
        m, j = divmod(b, lb)
        bx, by = (m % mw) * hs + j % hs, (m // mw) * vs + j // hs
        out[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = cache[key]
    return np.ascontiguousarray(out[:H, :W])


def decode(b):
    """-> (grey frame (H, W) uint8, number of bad intervals)"""
    coef, bad, g = coefficients(b)
    return frame_of(coef, g), len(bad)


_cache = {}


def reference(key, data):
    """(frame, coefficients, bad intervals, info) of a file, computed once per key"""
    if key not in _cache:
        coef, bad, g = coefficients(data)
        _cache[key] = (frame_of(coef, g), coef, bad, g)
    return _cache[key]

"""Principal components of the kept registered video, and which frames look like which, with nobody naming a cell.

Both come from one object, the Gram matrix of the frames G[i, j] = sum_p v_i(p) v_j(p), which the device makes on its
matrix cores as exact whole numbers (hm_body_rec_gram in include/hydra_mi.h, csrc/gram_kernels.h).  Everything else is host
arithmetic in NumPy on frames x frames numbers: exact whole numbers first, then one rounding each,
the rule of roi.footprints.

  gram              G (n, n) int64 and s1 (n,) uint64 of the frames k0 + i stride of the record
  centre            the Gram matrix of the video with every pixel's own temporal mean taken out
  components        its eigenvalues, temporal vectors and shares of the variance, largest first
  maps              every component's correlation image (network.maps of the temporal vectors)
  frame_similarity  Pearson's r over the pixels of every two frames
  frame_score       per frame the median r with the other frames: low where the track slipped
  pca               all of it in turn

    body = BodyReadout(kf, keep=True)
    ... track ...
    p = pca.pca(body, 4)
    p["share"], p["temporal"], p["rho"], p["frame_score"]

tests/pca_ref.py restates every step in loops and Python integers; the two agree bit for bit.
"""
import numpy as np

from . import network
from .body import BodyReadout

GRAM_MAX = 8192                       # the most frames hm_body_rec_gram takes (REC_GRAM_MAX)


def gram(body, k0=0, n=None, stride=1):
    """-> (G (n, n) int64, s1 (n,) uint64) of the frames k0 + i stride, i < n, of the record a BodyReadout(keep=True) has
    kept (n None: as many as there are from k0): G[i, j] the sum over the pixels of the product of frames i and j, s1[i]
    the sum of frame i.  Made on the device."""
    o = BodyReadout.record(body, "pca.gram").body_rec_gram(k0, n, stride)
    return o["G"], o["s1"]


def centre(G):
    """The Gram matrix (F, F) of whole numbers -> that of the video with every pixel's own mean over the F frames taken
    out, float64: (F^2 G_ij - F r_i - F r_j + t) / F^2, r the row sums and t the total.  The numerator is formed in int64
    and is exact while 4 F^2 max_i G_ii < 2^63 (each of its four terms is at most F^2 max G_ii: |G_ij| <= sqrt(G_ii G_jj);
    G_ii <= 65025 x the bytes of a frame); beyond that it raises with the numbers.  The numerator is rounded once to
    binary64, then one division by F^2."""
    G = np.asarray(G)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 1 or G.dtype.kind not in "iu":
        raise ValueError("pca.centre: a Gram matrix %s of shape %r (need whole numbers, frames x frames)" % (G.dtype, G.shape))
    F = G.shape[0]
    top = int(np.abs(G.diagonal()).max())
    if 4 * F * F * top >= 1 << 63:
        raise ValueError("pca.centre: 4 F^2 max G_ii = 4 x %d^2 x %d could pass 2^63" % (F, top))
    G = G.astype(np.int64)
    r = G.sum(1)
    t = r.sum()
    num = F * F * G - F * r[:, None] - F * r[None, :] + t
    return num.astype(np.float64) / np.float64(F * F)


def components(G, k):
    """The Gram matrix (F, F) -> (lam (k,), U (F, k), share (k,)): the k largest eigenvalues of centre(G) (numpy.linalg.eigh),
    descending and clipped at 0, their orthonormal temporal vectors, each signed so that its entry of largest magnitude (the
    first of them on ties) is positive, and lam / trace(centre(G)).  k is 1..F - 1 (the centred video has rank F - 1 at the
    most); a record of fewer than 2 frames raises."""
    F = np.shape(G)[0]
    if F < 2:
        raise ValueError("pca.components: %d frames (need at least 2)" % F)
    k = int(k)
    if not 1 <= k <= F - 1:
        raise ValueError("pca.components: %d components of %d frames (need 1..%d)" % (k, F, F - 1))
    Gc = centre(G)
    w, V = np.linalg.eigh(Gc)
    lam = np.maximum(w[::-1][:k], 0.0)
    U = np.ascontiguousarray(V[:, ::-1][:, :k])
    for c in range(k):
        if U[np.argmax(np.abs(U[:, c])), c] < 0.0:
            U[:, c] = -U[:, c]
    with np.errstate(invalid="ignore", divide="ignore"):
        share = lam / np.trace(Gc)
    return lam, U, share


def maps(body, U):
    """The temporal vectors (F, k) of all F recorded frames -> rho (k, H, W) float64: every component's correlation image,
    network.maps of the vectors as traces (NaN outside the map)."""
    U = np.asarray(U, np.float64)
    if U.ndim != 2:
        raise ValueError("pca.maps: temporal vectors of shape %r (need frames x components)" % (U.shape,))
    return network.maps(body, U.T)


def frame_similarity(G, s1, npix):
    """-> r (F, F) float64, Pearson's r over the npix pixels of the map of every two frames: C_ij = npix G_ij - s_i s_j in
    int64 (exact while 65025 npix^2 < 2^63, i.e. npix < 11 910 000: G_ij <= 65025 npix and s_i <= 255 npix; beyond that it
    raises), r_ij = C_ij / sqrt(C_ii C_jj): one rounding each, one product, one square root, one division.  NaN where a
    frame is constant."""
    G, s = np.asarray(G).astype(np.int64), np.asarray(s1).astype(np.int64)
    npix = int(npix)
    if G.ndim != 2 or G.shape[0] != G.shape[1] or s.shape != (G.shape[0],):
        raise ValueError("pca.frame_similarity: G of shape %r and s1 of shape %r" % (G.shape, s.shape))
    if npix < 1 or 65025 * npix * npix >= 1 << 63:
        raise ValueError("pca.frame_similarity: 65025 npix^2 = 65025 x %d^2 could pass 2^63 (or no pixel)" % npix)
    C = npix * G - s[:, None] * s[None, :]
    d = C.diagonal().astype(np.float64)
    flat = d == 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        r = C.astype(np.float64) / np.sqrt(d[:, None] * d[None, :])
    r[flat, :] = np.nan
    r[:, flat] = np.nan
    return r


def frame_score(r):
    """r (F, F) -> (F,) float64: per frame the median of r_ij over the j != i that are not NaN (of an even number, the two
    middle ones added and halved); NaN where there is none."""
    r = np.asarray(r, np.float64)
    F = r.shape[0]
    out = np.full(F, np.nan)
    for i in range(F):
        x = np.delete(r[i], i)
        x = np.sort(x[~np.isnan(x)])
        m = len(x)
        if m:
            out[i] = x[m // 2] if m % 2 else (x[m // 2 - 1] + x[m // 2]) / 2.0
    return out


def pca(body, k, k0=0, stride=1, frames=False):
    """All of it for the record of a BodyReadout(keep=True) -> dict: lam (k,), share (k,), temporal (F, k), rho (k, H, W),
    frame_score (F,), and with frames=True frame_r (F, F).  The maps multiply the temporal vectors into every frame of the
    record, so k0 and stride must be 0 and 1; for a subset of the frames use gram and components."""
    if int(k0) != 0 or int(stride) != 1:
        raise ValueError("pca.pca: the maps need every frame of the record (k0 0, stride 1), not k0 %d, stride %d: "
                         "gram and components take a subset" % (k0, stride))
    F = body.r.body_rec_count() if getattr(body, "keep", False) else 0
    if F > GRAM_MAX:
        raise ValueError("pca.pca: a record of %d frames, one Gram matrix takes %d at the most" % (F, GRAM_MAX))
    G, s1 = gram(body)
    lam, U, share = components(G, k)
    r = frame_similarity(G, s1, int((body.tri_of_pixel >= 0).sum()))
    out = dict(lam=lam, share=share, temporal=U, rho=maps(body, U), frame_score=frame_score(r))
    if frames:
        out["frame_r"] = r
    return out

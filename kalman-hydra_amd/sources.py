"""Host video input: whole videos as gray frames, and the frame sources ``pipeline.FlowEKFPipeline`` reads from.

Nothing here touches the GPU by itself (``load_video`` hands an MJPG file and 16-bit input to videoio / deepio, which
decode and map on the device when there is one).

``VideoStream`` mirrors reference renderer.py:739-805 on an array source (no OpenCV on this path):
``.npy`` / ``.npz`` of shape (frames, H, W) or (frames, H, W, 3), 8-bit.
"""
import numpy as np

from . import deepio
from .imgproc import findObjectThreshold
from .videoio import AviReader, decode_avi


def to_gray(a):
    """cv2.cvtColor(frame, COLOR_BGR2GRAY) for 8-bit frames (reference renderer.py:752,
    src/optical_flow_ext.cpp:366-368): rint(0.114 B + 0.587 G + 0.299 R).  2-D input is returned as is."""
    a = np.asarray(a)
    if a.ndim >= 3 and a.shape[-1] == 3:
        a = np.rint(0.114 * a[..., 0] + 0.587 * a[..., 1] + 0.299 * a[..., 2]).astype(np.uint8)
    return a


def load_video(fn, gray=True, depth=None):
    """The whole video as gray frames (frames, H, W) uint8 (gray=False: as read, (frames, H, W[, 3]) B G R) -- shared by run_kalmanfilter.py and
    optical_flow_ext.py, so that the tracker sees the frames its flow was computed on.  Sources (no OpenCV on this
    path; reference renderer.py:745 opens anything cv2.VideoCapture can): a NumPy ``.npy`` / ``.npz`` array of shape
    (frames, H, W[, 3]), a multi-page TIFF stack (``.tif`` / ``.tiff``, 8-bit gray or RGB pages, read with PIL), or an
    ``.avi`` (videoio.AviReader): Motion-JPEG frames are decoded on the device in runs (videoio.MjpegDecoder) and
    downloaded, uncompressed 24-bit frames are read on the host.  A Motion-JPEG file always gives gray frames, also with
    gray=False: a colour file's luma plane, which is libjpeg's gray output -- there is no colour decode.

    16-bit input (a ``uint16`` array, a TIFF stack of 16-bit gray pages; hydra_mi.deepio) is mapped to 8 bits through one
    window for the whole recording.  ``depth`` is None, {lo, hi, gamma} (the window itself) or {lo_ppm, hi_ppm, gamma}
    (the shares, in parts per million, that the window leaves below lo and keeps up to hi; defaults 1000 and 999 990,
    gamma 1).  Without lo and hi the window comes from the histogram of every pixel of every frame: a strided sample
    of the frames can miss the rare bright burst, which is the signal, and the window would then saturate exactly there.
    On a machine with a GPU the histogram and the mapping run on the device, without one in NumPy; the bytes are the
    same.  ``depth`` does nothing to 8-bit input, which takes the path it always took."""
    deep = deepio.load_deep(fn, depth)
    if deep is not None:
        if isinstance(deep["source"], deepio.TiffStack):
            deep["source"].close()
        return deep["frames"]
    if str(fn).lower().endswith(".avi"):
        with AviReader(fn) as reader:
            if len(reader) < 1:
                raise ValueError("%s: no frames" % fn)
            if reader.mjpeg:
                return decode_avi(reader)
            a = np.stack([reader.frame_bgr(f) for f in range(len(reader))])
        return np.ascontiguousarray(to_gray(a) if gray else a)
    if str(fn).lower().endswith((".tif", ".tiff")):
        from PIL import Image, ImageSequence                      # (no cycle: PIL is needed for TIFF only, as in videoio)
        with Image.open(fn) as im:
            pages = []
            for page in ImageSequence.Iterator(im):
                if page.mode not in ("L", "RGB"):
                    raise ValueError("%s: expected 8-bit gray or RGB pages, found mode %s" % (fn, page.mode))
                a = np.asarray(page)
                pages.append(a[..., ::-1] if a.ndim == 3 else a)          # RGB -> BGR, the order cv2 hands out
        if not pages or any(p.shape != pages[0].shape for p in pages):
            raise ValueError("%s: expected pages of one size" % fn)
        a = np.stack(pages)
    else:
        a = np.load(fn)
        if hasattr(a, "files"):
            a = a[a.files[0]]
        a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or (a.ndim == 4 and a.shape[-1] != 3):
        raise ValueError("%s: expected an 8-bit array of shape (frames, H, W[, 3])" % fn)
    return np.ascontiguousarray(to_gray(a) if gray else a)


def threshold_mask(gray, threshold):
    """The mask imgproc.findObjectThreshold returns (reference imgproc.py:195-197): intensity above threshold."""
    return (np.asarray(gray) > threshold).astype(np.uint8)


class VideoStream:
    """reference renderer.py:739-805 over an in-memory frame stack."""

    def __init__(self, fn, threshold):
        self.threshold = threshold
        self.frames = load_video(fn) if isinstance(fn, str) else np.ascontiguousarray(to_gray(np.asarray(fn)))
        if self.frames.shape[0] < 1:
            raise ValueError("Cannot open %s" % (fn,))
        self.pos = 0
        self.nx, self.ny = self.frames.shape[1:3]
        self.frame = self.frames[0]
        self.frame_orig = self.frame.copy()
        self.grayframe = self.frame

    def read(self, backsub=True):
        """-> (ret, frame, grayframe, mask) with the background removed, or (ret, frame, grayframe)."""
        if self.pos + 1 >= self.frames.shape[0]:
            self.pos = self.frames.shape[0]
            return False, None, None, None
        self.pos += 1
        self.frame = self.grayframe = self.frames[self.pos]
        if not backsub:
            return True, self.frame, self.grayframe
        mask = threshold_mask(self.frame, self.threshold)
        back = mask * self.frame
        return True, back, back, mask

    def current_frame(self, backsub=True):
        return threshold_mask(self.frame, self.threshold) * self.frame if backsub else self.frame

    gray_frame = current_frame

    def backsub(self, im=None):
        if im is None:                                 # (mask, contours, signed distance function): DistMesh's input
            return findObjectThreshold(self.frame, threshold=self.threshold)
        mask = threshold_mask(self.frame, self.threshold)
        im = np.asarray(im)
        return mask * im if im.ndim == 2 else mask[:, :, None] * im

    def isOpened(self):
        return self.pos < self.frames.shape[0]

    # frame source protocol of FlowEKFPipeline: random access to (raw frame, mask, frame shown to the filter)
    def __len__(self):
        return self.frames.shape[0]

    @property
    def shape(self):
        return self.frames.shape[1:3]

    def frame_at(self, f):
        fr = self.frames[f]
        mask = threshold_mask(fr, self.threshold)
        return fr, mask, mask * fr

    def release(self):
        self.pos = self.frames.shape[0]


class ArraySource:
    """Frame source over host arrays: video, masks (frames, H, W) uint8, optionally the frames the filter is
    shown when they differ from the ones the flow is computed on."""

    def __init__(self, video, masks, observed=None):
        video = np.ascontiguousarray(video, np.uint8)
        masks = np.ascontiguousarray(masks, np.uint8)
        if video.ndim != 3 or masks.shape != video.shape:
            raise ValueError("video and masks must both be (frames, H, W) uint8")
        if observed is not None:
            observed = np.ascontiguousarray(observed, np.uint8)
            if observed.shape != video.shape:
                raise ValueError("observed must have the shape of video")
        self.video, self.masks, self.observed = video, masks, observed

    def __len__(self):
        return self.video.shape[0]

    @property
    def shape(self):
        return self.video.shape[1:3]

    def frame_at(self, f):
        return self.video[f], self.masks[f], None if self.observed is None else self.observed[f]

"""``DeviceBuffer``: a block of device memory that the Python side owns."""
import numpy as np

from . import _lib


class DeviceBuffer:
    """A block of device memory owned by the caller side of the C-ABI (hm_dev_alloc)."""

    def __init__(self, nbytes, device=0):
        self.device, self.nbytes = int(device), int(nbytes)
        p = _lib.c_vp()
        _lib.check(_lib.lib().hm_dev_alloc(self.device, self.nbytes, p), "hm_dev_alloc")
        self.ptr = p.value
        _lib.register(self, 4)

    def upload(self, a, offset=0):
        a = np.ascontiguousarray(a)
        assert offset + a.nbytes <= self.nbytes
        _lib.check(_lib.lib().hm_dev_upload(self.device, self.ptr + offset, _lib.ptr(a), a.nbytes), "hm_dev_upload")

    def download(self, out, offset=0):
        assert out.flags["C_CONTIGUOUS"] and offset + out.nbytes <= self.nbytes
        _lib.check(_lib.lib().hm_dev_download(self.device, _lib.ptr(out), self.ptr + offset, out.nbytes), "hm_dev_download")
        return out

    def close(self):
        if getattr(self, "ptr", None):
            _lib.lib().hm_dev_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

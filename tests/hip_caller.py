"""A caller's side of the _device entry points for the GPU tests: a HIP stream of its own, from the HIP runtime libfskhip.so has
loaded into this process, and device buffers from fskhip_device_malloc that are filled and read back through the library."""
import ctypes as C

import numpy as np


def hip_runtime():
    """the HIP runtime libfskhip.so has loaded into this process (found in the process's own map, so that it is that copy)"""
    with open("/proc/self/maps") as fh:
        paths = {line.split()[-1] for line in fh if "libamdhip64.so" in line and "/torch/" not in line}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipStreamCreate.argtypes, hip.hipStreamSynchronize.argtypes, hip.hipStreamDestroy.argtypes = [C.POINTER(C.c_void_p)], [C.c_void_p], [C.c_void_p]
    return hip


class Caller:
    def __init__(self, engine):
        from webaudio_modem_amd import _lib
        self._lib, self.L, self.e = _lib, _lib.lib(), engine._h
        self.hip, self.stream, self.bufs = hip_runtime(), C.c_void_p(), []
        assert self.hip.hipStreamCreate(C.byref(self.stream)) == 0 and self.stream.value

    def malloc(self, nbytes):
        d = C.c_void_p()
        self._lib.check(self.L.fskhip_device_malloc(self.e, nbytes, C.byref(d)))
        self.bufs.append(d)
        return d.value

    def upload(self, d, a):
        a = np.ascontiguousarray(a)
        self._lib.check(self.L.fskhip_memcpy_h2d(self.e, d, a.ctypes.data, a.nbytes))

    def download(self, d, a):
        self._lib.check(self.L.fskhip_memcpy_d2h(self.e, a.ctypes.data, d, a.nbytes))
        return a

    def sync(self):
        assert self.hip.hipStreamSynchronize(self.stream) == 0

    def close(self):
        for d in self.bufs:
            self._lib.check(self.L.fskhip_device_free(self.e, d))
        assert self.hip.hipStreamDestroy(self.stream) == 0

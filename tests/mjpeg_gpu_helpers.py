"""Helpers the GPU tests of the Motion-JPEG readers share (tests/test_gpu_mjpeg_sync.py; tests/test_gpu_mjpeg_read.py keeps its own,
older copies): the current stream, a host byte array for the C ABI, guarded int64 cells, and the search for one changed bit that the
restatement answers in a given way."""
import ctypes as C

import torch

from hunyuanvideo_efficiency_amd import mjpeg_io
from tests import mjpeg_read_ref as D
from tests.guarded_memory import GuardedFlat

DEV = "cuda:0"


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def _u8(values):
    return C.cast((C.c_uint8 * len(values))(*values), C.c_void_p)


class _Guarded64:
    """n int64 cells behind 16 bytes of sentinel and in front of 256 more (tests/guarded_memory.py has no 8-byte cells)"""

    def __init__(self, n):
        self.g = GuardedFlat(2 * n, torch.int32, front=4)
        self.view = self.g.view.view(torch.int64)

    def intact(self):
        return self.g.intact()


def _first_bad_flip(d, p, lo=None, hi=None, accept=lambda status, found: any(status)):
    """the first single-bit change in [lo, hi) (default: the second half of the scan) that leaves the frame parseable with the same scan
    and that the restatement answers with a (status list, found word) `accept` takes"""
    lo, hi = (p["begin"] + p["end"]) // 2 if lo is None else lo, p["end"] if hi is None else hi
    for pos in range(lo, hi):
        m = bytearray(d)
        m[pos] ^= 0x10
        m = bytes(m)
        try:
            q = D.parse(m)
            fr = mjpeg_io.parse_jpeg(m)
        except ValueError:
            continue                                     # the change made a marker: the parsers refuse the frame, nothing to decode
        if (q["begin"], q["end"]) == (p["begin"], p["end"]) == (fr.scan_begin, fr.scan_end):
            _, status, found = D.decode_coefs(m, q)
            if accept(status, found):
                return m
    raise AssertionError("no such change of one bit")

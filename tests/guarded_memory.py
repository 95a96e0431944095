"""Poisoned operands and guarded outputs for the GPU edge tests: an operand is embedded in NaN-filled memory (rows before and after it,
columns behind its width), an output in a sentinel-filled buffer whose cells outside the view must keep their bits.
Every helper takes `device` (default: the GPU), so that tests/double_parity.py builds the same case for a kernel and for its CPU double."""
import torch

DEV = "cuda"
SENT = {2: 0x7E5A, 4: 0x7F5A5A5A}            # sentinel bit patterns of 16- and 32-bit output cells
INT = {2: torch.int16, 4: torch.int32, 1: torch.uint8}
NAN_BITS = {4: 0x7FC00000, 2: 0x7FFF, 1: 0x7F}   # a NaN in fp32, in bf16 and fp16 (0x7FFF), in e4m3fn (0x7F)


class Poisoned:
    """t [R, C] placed at rows [before, before + R), columns [0, C) of a NaN-filled [before + R + after, C + pad] buffer"""

    def __init__(self, t, before=3, after=5, pad=24, device=DEV):
        es = t.element_size()
        R_, C_ = t.shape
        self.buf = torch.full((before + R_ + after, C_ + pad), NAN_BITS[es], dtype=INT[es], device=device)
        self.view = self.buf.view(t.dtype)[before:before + R_, :C_]
        self.view.copy_(t)
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[before:before + R_, :C_] = False

    def intact(self):
        return bool((self.buf[self.mask] == NAN_BITS[self.buf.element_size()]).all())


def poisoned_vec(v, after=24, device=DEV):
    """a contiguous vector followed by NaNs"""
    es = v.element_size()
    buf = torch.full((v.numel() + after,), NAN_BITS[es], dtype=INT[es], device=device).view(v.dtype)
    buf[:v.numel()].copy_(v)
    return buf[:v.numel()]


class Guarded:
    """an output [M, n] at rows [before, before + M), columns [c0, c0 + n) of a sentinel-filled buffer"""

    def __init__(self, M, n, dtype, c0=0, before=2, after=3, pad=16, device=DEV):
        es = torch.empty((), dtype=dtype).element_size()
        self.sent = SENT[es]
        self.buf = torch.full((before + M + after, c0 + n + pad), self.sent, dtype=INT[es], device=device)
        self.view = self.buf.view(dtype)[before:before + M, c0:c0 + n]
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[before:before + M, c0:c0 + n] = False

    def intact(self):
        return bool((self.buf[self.mask] == self.sent).all())


def bits(t):
    return t.contiguous().view(INT[t.element_size()])


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class GuardedFlat:
    """a contiguous output of n elements behind `front` sentinel elements (a multiple of 16 bytes, so that the view keeps the alignment
    of an allocation) and in front of 64 more"""

    def __init__(self, n, dtype, front=None, device=DEV):
        es = torch.empty((), dtype=dtype).element_size()
        front = 16 // es * 2 if front is None else front
        self.sent = SENT.get(es, 0x5A)
        self.buf = torch.full((front + n + 64,), self.sent, dtype=INT[es], device=device)
        self.view = self.buf.view(dtype)[front:front + n]
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[front:front + n] = False

    def intact(self):
        return bool((self.buf[self.mask] == self.sent).all())


class GuardedBytes:
    """fp8 rows [M, D] with row stride ldq bytes inside a 0x5A-filled byte buffer"""

    def __init__(self, M, D, ldq, before=2, after=3, device=DEV):
        self.buf = torch.full((before + M + after, ldq), 0x5A, dtype=torch.uint8, device=device)
        self.view = self.buf.view(torch.float8_e4m3fn)[before:before + M, :D]
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask[before:before + M, :D] = False

    def intact(self):
        return bool((self.buf[self.mask] == 0x5A).all())


def crop(shape, dtype, key, margin=(1, 2, 1, 3), poison=True, device=DEV):
    """a [C,T,H,W] view inside a larger NaN-filled (or sentinel-filled) tensor; returns (buffer, view, mask of the cells outside the view)"""
    big = [s + 2 * m for s, m in zip(shape, margin)]
    es = torch.empty((), dtype=dtype).element_size()
    fill = NAN_BITS[es] if poison else SENT[es]
    buf = torch.full(big, fill, dtype=INT[es], device=device)
    sl = tuple(slice(m, m + s) for s, m in zip(shape, margin))
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[sl] = False
    return buf, buf.view(dtype)[sl], mask

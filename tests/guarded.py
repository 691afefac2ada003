"""Output buffers with guard bands for the GPU form tests that call the C ABI directly (a helper, not a test): the NaN-guarded
views of tests/test_gpu_glue_forms.py.  An element the kernel never wrote stays NaN and fails any comparison; a store past
either end of the output lands in a guard band, which ``untouched()`` finds."""
import ctypes

import torch

GUARD = 64                        # floats on each side: 256 bytes, so the view keeps the buffer's 16-byte alignment
NAN = float("nan")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Guarded(object):
    """``rows`` x ``cols`` floats (row stride ``stride`` >= cols) as ``view`` into a NaN-filled CUDA buffer with GUARD floats
    before and behind; ``fill``: what the view itself starts as (NaN unless given).  With stride > cols the floats between the
    rows are guards as well."""

    def __init__(self, rows, cols, stride=None, fill=None):
        stride = cols if stride is None else stride
        assert stride >= cols
        self.rows, self.cols, self.stride = rows, cols, stride
        self.buf = torch.full((GUARD + rows * stride + GUARD,), NAN, device="cuda")
        self.view = self.buf[GUARD:GUARD + rows * stride].view(rows, stride)[:, :cols]
        if fill is not None:
            self.view.copy_(fill.reshape(rows, cols) if torch.is_tensor(fill) else torch.full((rows, cols), float(fill)))
        inside = torch.zeros(GUARD + rows * stride + GUARD, dtype=torch.bool)
        inside[GUARD:GUARD + rows * stride].view(rows, stride)[:, :cols] = True
        self.outside = (~inside).cuda()
        assert self.view.data_ptr() % 16 == 0

    def untouched(self):
        return bool(torch.isnan(self.buf[self.outside]).all())

    def all_nan(self):
        return bool(torch.isnan(self.buf).all())


def view_of(g):
    return None if g is None else g.view

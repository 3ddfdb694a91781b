"""What the direct kernel tests (test_gpu_kernels_direct.py, test_gpu_bn_direct.py) share: guarded NaN-prefilled device buffers,
the worst error / bound ratio over all elements, and the record of the worst ratio per family."""
import numpy as np
import torch

GUARD = 256               # elements after every buffer


class Buf:
    """a device buffer of ``shape`` followed by GUARD elements; both start as NaN (a bit pattern for integers and bytes)"""

    def __init__(self, shape, dtype=torch.float32, init=None):
        self.n = int(np.prod(shape))
        self.flat = torch.empty(self.n + GUARD, dtype=dtype, device='cuda')
        self.pattern = None if dtype.is_floating_point else (0xA5 if dtype == torch.uint8 else 0x5A5A5A5A)
        self.flat.fill_(float('nan') if self.pattern is None else self.pattern)
        self.t = self.flat[:self.n].view(*shape)
        if init is not None:
            self.t.copy_(init if torch.is_tensor(init) else torch.from_numpy(np.ascontiguousarray(init)))

    def guard_ok(self):
        g = self.flat[self.n:]
        return bool(torch.isnan(g).all()) if self.pattern is None else bool((g == self.pattern).all())

    def np(self):
        """the body on the host: fp32 as is, bf16 as float32 (exact)"""
        return self.t.float().cpu().numpy() if self.t.dtype == torch.bfloat16 else self.t.cpu().numpy()

    def bits(self):
        return self.t.view(torch.int16).cpu().numpy().view(np.uint16)


def ratio(got, ref, bound):
    """worst |got - ref| / bound over ALL elements (0/0 counts as 0, a non-finite or unexplained error as inf)"""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    err = np.where(np.isfinite(got), err, np.inf)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


WORST = {}


def record(family, case, r):
    WORST[family] = max(WORST.get(family, 0.0), r)
    print(f'RATIO {family} {case}: {r:.4f}   (worst so far {WORST[family]:.4f})')
    return r


def p(L, b):
    return None if b is None else L.ptr(b.t if isinstance(b, Buf) else b)


def guards(*bufs):
    return all(b.guard_ok() for b in bufs if b is not None)


def last_error(L):
    m = L.lib.w2l_last_error()
    return m.decode() if m else ''

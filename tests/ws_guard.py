"""TEST INFRASTRUCTURE ONLY - guarded, poisoned workspaces for the entries that take a caller-owned scratch buffer.

Every workspace of the package is obtained through a module-level `_ws(nbytes, device)` helper (dense2d, dense3d, hip_ops - which
also has `_ws_shared` - nms, anchors, prep, solver).  `guard(monkeypatch, poison)` replaces all of them for the length of a `with`
block.  A request of `nbytes` becomes

    [ front guard 4096 B | n bytes handed to the entry | back guard max(4096, min(n, 1 MiB)) B ]

with n = max(nbytes, floor) - the floor the real helper applies when it allocates exactly (256 where it has one; the 1 MiB minimum
of dense2d's shared buffer is NOT reproduced: the exact-size allocation it makes while a HIP graph is captured is the case to
hold).  The whole allocation is filled with one poison byte, the middle slice is 256-byte aligned and has numel() == n, so an
entry's own size check sees exactly what its query asked for.  On exit, after a device synchronise, both guards of every request
must still hold the poison: an entry touches only the bytes its query asked for.  Running a case under two poisons (0xFF: NaN as
fp32 / bf16, -1 as an integer; 0x5A: ~1.5e16, finite, a large positive integer) and comparing the results checks the other
invariant: an entry writes every scratch word before it reads it.  Zero is no poison - it hides missing zero-fills.

Eager calls only: a request made while a HIP graph is being captured raises."""
import contextlib
import importlib

import torch

FRONT = 4096
BACK_MIN = 4096
BACK_MAX = 1 << 20
ALIGN = 256
POISONS = (0xFF, 0x5A)

# (module, attribute, floor applied to the requested size)
SEAMS = (("dense2d", "_ws", 256), ("dense3d", "_ws", 256), ("hip_ops", "_ws", 256), ("hip_ops", "_ws_shared", 256),
         ("nms", "_ws", 0), ("anchors", "_ws", 0), ("prep", "_ws", 0), ("solver", "_ws", 0))


class GuardViolation(AssertionError):
    pass


class GuardLog:
    """the requests made inside one `guard` block: .requests = [(module, n)], every allocation kept alive until the block exits"""

    def __init__(self, poison):
        assert poison in POISONS, f"poison byte {poison:#x}: one of {[hex(p) for p in POISONS]} (zero hides missing zero-fills)"
        self.poison = poison
        self.requests = []
        self._allocs = []   # (module, n, base, start): the guards are base[start - FRONT:start] and base[start + n:start + n + back]

    def modules(self):
        return {m for m, _ in self.requests}

    def alloc(self, module, nbytes, device, floor=0):
        device = torch.device(device)
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ws_guard: eager calls only - a workspace was requested while a HIP graph is being captured")
        n = max(int(nbytes), int(floor))
        back = max(BACK_MIN, min(n, BACK_MAX))
        base = torch.full((ALIGN + FRONT + n + back,), self.poison, dtype=torch.uint8, device=device)
        start = FRONT + (-(base.data_ptr() + FRONT)) % ALIGN
        ws = base[start:start + n]
        assert ws.numel() == n and (n == 0 or ws.data_ptr() % ALIGN == 0)
        self.requests.append((module, n))
        self._allocs.append((module, n, base, start, back))
        return ws

    def check(self):
        """both guards of every request still hold the poison (call after the device is idle)"""
        for module, n, base, start, back in self._allocs:
            for side, lo, hi in (("front", start - FRONT, start), ("back", start + n, start + n + back)):
                bad = (base[lo:hi] != self.poison).nonzero()
                if bad.numel():
                    first = int(bad[0]) + lo - start
                    where = f"{-first} bytes in front of" if side == "front" else f"byte {first - n} past the end of"
                    raise GuardViolation(f"{module}: the {side} guard of a {n}-byte workspace was overwritten ({int(bad.numel())} bytes, the "
                                         f"first {where} the buffer; poison {self.poison:#x})")


@contextlib.contextmanager
def guard(monkeypatch, poison):
    """`with guard(monkeypatch, 0xFF) as log:` - every workspace requested inside the block is guarded and poisoned; the guards are
    checked when the block ends normally, the seams are restored either way."""
    log = GuardLog(poison)
    with monkeypatch.context() as mp:
        for module, attr, floor in SEAMS:
            mod = importlib.import_module("sparse2dense_amd." + module)
            assert callable(getattr(mod, attr)), (module, attr)
            mp.setattr(mod, attr, lambda nbytes, device, _m=module, _f=floor: log.alloc(_m, nbytes, device, _f))
        yield log
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    log.check()

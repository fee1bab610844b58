"""TEST INFRASTRUCTURE ONLY - calls the twelve s2d_convt3d_mfma_* entries through the C ABI into caller-owned, poisoned, guarded buffers
(tests/ws_guard.py) and measures them against tests/convt3d_ref.py.  Used by tests/test_convt3d_variants_gpu.py in process.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import convt3d_ref as R   # noqa: E402
import ws_guard           # noqa: E402

DEV = "cuda:0"
POISON = 0xFF   # NaN as fp32 and as bf16

FWD = ("fwd", "fwd_stats", "fwd_stats_y16", "fwd_stats_y16_norm", "fwd_stats_y16_norm_x16")
DGRAD = ("dgrad", "dgrad_d16", "dgrad_d16_x16")
WGRAD = ("wgrad", "wgrad_d16", "wgrad_d16_norm", "wgrad_d16_norm_x16")


def _lib():
    from sparse2dense_amd import _lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def predicate(lib, entry, cin, cout, shp):
    """the `*_supported` predicate that governs an entry"""
    n, d, h, w = shp
    if entry.endswith("_x16"):
        return bool(lib.s2d_convt3d_mfma_x16_supported(cin, cout, d, h, w))
    if "_norm" in entry:
        return bool(lib.s2d_convt3d_mfma_norm_supported(cin, cout, d, h, w))
    if "_d16" in entry:
        return bool(lib.s2d_convt3d_mfma_d16_supported(cin, cout, d, h, w))
    return bool(lib.s2d_convt3d_mfma_supported(cin, cout))


class DeviceCase:
    """the device copies of one convt3d_ref.case: every storage form of x and dout, scale | shift, the packed weight images"""

    def __init__(self, c):
        lib = _lib()
        self.c, self.cin, self.cout, self.shape = c, c["cin"], c["cout"], c["shape"]
        up = lambda t: t.contiguous().to(DEV)
        self.x, self.dout, self.bias = up(c["x"]), up(c["dout"]), up(c["bias"])
        self.ss = up(torch.cat([c["scale"], c["shift"]]))
        if c["rounded"]:   # bf16-representable: the bf16-stored forms hold the same values
            self.x16, self.xn = up(c["x"].to(torch.bfloat16)), up(c["xn"])
        self.dout16 = up(c["dout"].to(torch.bfloat16))   # torch's round to nearest even
        self.dout16w = self.dout16.float()               # ... widened back
        w = up(c["w"])
        self.packed = torch.empty(lib.s2d_convt3d_mfma_packed_elems(self.cin, self.cout), dtype=torch.bfloat16, device=DEV)
        assert self.packed.numel() > 0
        rc = lib.s2d_convt3d_mfma_pack_weights(w.data_ptr(), self.cin, self.cout, self.packed.data_ptr(), _stream())
        assert rc == 0, rc
        self.tiles = int(lib.s2d_convt3d_mfma_stats_tiles(self.shape[0], self.cin, *self.shape[1:]))
        self.ws_bytes = int(lib.s2d_convt3d_mfma_wgrad_workspace_bytes(self.shape[0], self.cin, self.cout, *self.shape[1:]))

    def dims(self):
        n, d, h, w = self.shape
        return (n, self.cin, self.cout, d, h, w)


def alloc(log, shape, dtype):
    numel = 1
    for s in shape:
        numel *= int(s)
    esize = torch.empty((), dtype=dtype).element_size()
    return log.alloc("convt3d", numel * esize, DEV).view(dtype).view(*shape)


def call_fwd(lib, log, dc, entry, x):
    """-> (rc, out, stats | None) with out / stats poisoned before the call"""
    n, d, h, w = dc.shape
    out = alloc(log, (n, dc.cout, 2 * d, 2 * h, 2 * w), torch.bfloat16 if "y16" in entry else torch.float32)
    stats = None if entry == "fwd" else alloc(log, (dc.tiles, 2, dc.cout), torch.float32)
    fn = getattr(lib, "s2d_convt3d_mfma_" + entry)
    head = (x.data_ptr(), dc.ss.data_ptr()) if "_norm" in entry else (x.data_ptr(),)
    tail = (out.data_ptr(), _stream()) if stats is None else (out.data_ptr(), stats.data_ptr(), _stream())
    rc = fn(*head, dc.packed.data_ptr(), dc.bias.data_ptr(), *dc.dims(), *tail)
    return rc, out, stats


def call_dgrad(lib, log, dc, entry, dout):
    n, d, h, w = dc.shape
    din = alloc(log, (n, dc.cin, d, h, w), torch.bfloat16 if entry.endswith("_x16") else torch.float32)
    rc = getattr(lib, "s2d_convt3d_mfma_" + entry)(dout.data_ptr(), dc.packed.data_ptr(), *dc.dims(), din.data_ptr(), _stream())
    return rc, din


def call_wgrad(lib, log, dc, entry, x, dout):
    dw = alloc(log, (dc.cin, dc.cout, 4, 4, 4), torch.float32)
    ws = log.alloc("convt3d", dc.ws_bytes, DEV)   # exactly what the query asks for, poisoned, guarded
    head = (x.data_ptr(), dc.ss.data_ptr(), dout.data_ptr()) if "_norm" in entry else (x.data_ptr(), dout.data_ptr())
    rc = getattr(lib, "s2d_convt3d_mfma_" + entry)(*head, *dc.dims(), dw.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
    return rc, dw


def _refused(rep, tag, rc, buffers, poison):
    rep.rc(f"{tag} refuses", rc, R.S2D_ERR_UNSUPPORTED)
    torch.cuda.synchronize()
    rep.untouched(f"{tag} outputs untouched", [b for b in buffers if b is not None], poison)


def _finish(rep, log):
    torch.cuda.synchronize()
    rep.guards("guards", log)


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
def forward_case(dc, rep):
    """every forward entry on one shape: float64 bars, the epilogue statistics and the bit identities; refusals where the predicate says no"""
    lib, c = _lib(), dc.c
    log = ws_guard.GuardLog(POISON)
    ok = {e: predicate(lib, e, dc.cin, dc.cout, dc.shape) for e in FWD}
    got = {}
    for e in FWD:
        if not c["rounded"] and "_norm" in e:
            continue   # the unrounded inputs are for the forms without the fold
        x = dc.x16 if e.endswith("_x16") else dc.x
        rc, out, stats = call_fwd(lib, log, dc, e, x)
        if not ok[e]:
            _refused(rep, e, rc, [out, stats], POISON)
            continue
        rep.rc(f"{e} rc", rc, R.S2D_OK)
        torch.cuda.synchronize()
        got[e] = (out.cpu(), None if stats is None else stats.cpu())
    # the plain form fed the pre-normalised tensor (exact on the host): what the fold must reproduce bit for bit
    if "fwd_stats_y16_norm" in got:
        rc, out, stats = call_fwd(lib, log, dc, "fwd_stats_y16", dc.xn)
        rep.rc("fwd_stats_y16(xn) rc", rc, R.S2D_OK)
        torch.cuda.synchronize()
        got["prenorm"] = (out.cpu(), stats.cpu())
    _finish(rep, log)
    for e, (out, stats) in got.items():
        ref = c["yn"] if ("_norm" in e or e == "prenorm") else c["y"]
        (rep.bf16 if out.dtype == torch.bfloat16 else rep.f32)(f"{e} y", out, ref)
        if stats is not None:
            rep.stats(f"{e} stats", stats, out, dc.tiles)
    if "fwd" in got and "fwd_stats" in got:
        rep.same("fwd == fwd_stats", got["fwd"][0], got["fwd_stats"][0])
    if "fwd_stats_y16" in got and "fwd_stats" in got:
        rep.same("y16 == bf16(y32)", got["fwd_stats_y16"][0], got["fwd_stats"][0].to(torch.bfloat16))
    if "prenorm" in got:
        rep.same("y16_norm(x) == y16(relu(x * scale + shift))", got["fwd_stats_y16_norm"][0], got["prenorm"][0])
        rep.same("y16_norm(x) stats == y16(relu(x * scale + shift)) stats", got["fwd_stats_y16_norm"][1], got["prenorm"][1])
    if "fwd_stats_y16_norm_x16" in got:
        rep.same("y16_norm_x16 == y16_norm", got["fwd_stats_y16_norm_x16"][0], got["fwd_stats_y16_norm"][0])
        rep.same("y16_norm_x16 stats == y16_norm stats", got["fwd_stats_y16_norm_x16"][1], got["fwd_stats_y16_norm"][1])
    return got


# ---- data gradient ----------------------------------------------------------------------------------------------------------------------
def dgrad_case(dc, rep):
    lib, c = _lib(), dc.c
    log = ws_guard.GuardLog(POISON)
    got = {}
    for e in DGRAD:
        rc, din = call_dgrad(lib, log, dc, e, dc.dout if e == "dgrad" else dc.dout16)
        if not predicate(lib, e, dc.cin, dc.cout, dc.shape):
            _refused(rep, e, rc, [din], POISON)
            continue
        rep.rc(f"{e} rc", rc, R.S2D_OK)
        torch.cuda.synchronize()
        got[e] = din.cpu()
    if not c["rounded"]:   # the fp32 form fed the values torch rounded, widened: the d16 identity's other side
        rc, din = call_dgrad(lib, log, dc, "dgrad", dc.dout16w)
        rep.rc("dgrad(widened) rc", rc, R.S2D_OK)
        torch.cuda.synchronize()
        got["widened"] = din.cpu()
    _finish(rep, log)
    for e, din in got.items():
        (rep.bf16 if din.dtype == torch.bfloat16 else rep.f32)(f"{e} din", din, c["din"])
    if "dgrad_d16" in got:
        rep.same("dgrad_d16(bf16 dout) == dgrad(widened)", got["dgrad_d16"], got.get("widened", got["dgrad"]))
        if "widened" in got:
            rep.same("dgrad(fp32 dout) == dgrad_d16(torch-rounded dout): round to nearest even on load", got["dgrad"], got["dgrad_d16"])
    if "dgrad_d16_x16" in got:
        rep.same("din of dgrad_d16_x16 == bf16(din of dgrad_d16)", got["dgrad_d16_x16"], got["dgrad_d16"].to(torch.bfloat16))
    return got


# ---- weight gradient --------------------------------------------------------------------------------------------------------------------
def wgrad_case(dc, rep):
    """every weight-gradient entry under both poisons of the scratch: equal results (scratch is written before it is read)"""
    lib, c = _lib(), dc.c
    runs = {}
    for poison in ws_guard.POISONS:
        log = ws_guard.GuardLog(poison)
        got = {}
        for e in WGRAD:
            if not c["rounded"] and "_norm" in e:
                continue
            x = dc.x16 if e.endswith("_x16") else dc.x
            rc, dw = call_wgrad(lib, log, dc, e, x, dc.dout if e == "wgrad" else dc.dout16)
            if not predicate(lib, e, dc.cin, dc.cout, dc.shape):
                _refused(rep, f"{e} [{poison:#x}]", rc, [dw], poison)
                continue
            rep.rc(f"{e} [{poison:#x}] rc", rc, R.S2D_OK)
            torch.cuda.synchronize()
            got[e] = dw.cpu()
        if "wgrad_d16_norm" in got:
            rc, dw = call_wgrad(lib, log, dc, "wgrad_d16", dc.xn, dc.dout16)
            rep.rc("wgrad_d16(xn) rc", rc, R.S2D_OK)
            torch.cuda.synchronize()
            got["prenorm"] = dw.cpu()
        if not c["rounded"]:
            rc, dw = call_wgrad(lib, log, dc, "wgrad", dc.x, dc.dout16w)
            rep.rc("wgrad(widened) rc", rc, R.S2D_OK)
            torch.cuda.synchronize()
            got["widened"] = dw.cpu()
        _finish(rep, log)
        runs[poison] = got
    a, b = (runs[p] for p in ws_guard.POISONS)
    for e, dw in a.items():
        rep.f32(f"{e} dW", dw, c["dwn"] if ("_norm" in e or e == "prenorm") else c["dw"])
        rep.same(f"{e} dW under both scratch poisons", dw, b[e])
    if "wgrad_d16" in a:
        rep.same("wgrad_d16(bf16 dout) == wgrad(widened)", a["wgrad_d16"], a.get("widened", a["wgrad"]))
        if "widened" in a:
            rep.same("wgrad(fp32 dout) == wgrad_d16(torch-rounded dout): round to nearest even on load", a["wgrad"], a["wgrad_d16"])
    if "prenorm" in a:
        rep.same("wgrad_d16_norm(x) == wgrad_d16(relu(x * scale + shift))", a["wgrad_d16_norm"], a["prenorm"])
    if "wgrad_d16_norm_x16" in a:
        rep.same("wgrad_d16_norm_x16 == wgrad_d16_norm", a["wgrad_d16_norm_x16"], a["wgrad_d16_norm"])
    return a

"""TEST INFRASTRUCTURE ONLY - the float64 reference, the inputs and the checks of the ConvTranspose3d(4, 2, 1) matrix-core entries
(csrc/convt3d_mfma.hip).  Host only: nothing here touches a GPU, tests/test_convt3d_variants_checks_cpu.py runs every check on the host.

Operand model.  Every entry multiplies bf16 operands and accumulates in fp32:
    x operand     bf16(x), or with the norm fold bf16(relu(x * scale[ci] + shift[ci])); padding cells are zero AFTER the normalisation
    weight        bf16(w)
    dout operand  bf16(dout)
The reference is torch's conv_transpose3d(stride 2, padding 1) and its autograd gradients in float64 on the CPU over exactly these
operands, rounded with torch (`.to(torch.bfloat16)`, round to nearest even).

Inputs.  The `rounded` inputs make the norm fold exact: x is a multiple of 1/32 in [-4, 4] (8 significant bits: bf16-representable),
scale a multiple of 1/8 in [0.5, 1.5], shift a multiple of 1/16 in [-0.5, 0.5] - x * scale + shift is a multiple of 1/256 below 8, exact in
fp32, so the float64 host value IS what the kernel's fp32 fma forms; its rounding to bf16 then meets ties in quantity (round to nearest
EVEN is exercised, not only round to nearest).  Every even channel has shift > 0: a padding cell that is normalised instead of zeroed
contributes bf16(relu(shift)) != 0.  dout and w are bf16(randn).  The `unrounded` inputs are plain fp32 randn for x, w and dout: the
reference rounds them with torch, which pins the rounding mode of the kernels' loads.

Bars.
    fp32-stored results (y, din, dW):       max |got - ref| <= 1e-4 * max |ref|       (K <= 256 products per output, <= ~1e6 per dW entry:
                                            fp32 accumulation order is all that is left; the bar of test_convtranspose3d_bf16_mfma)
    bf16-stored results (y16, din of x16):  |got - ref| <= 2^-8 * |ref| + 1e-4 * max |ref| elementwise (2^-8 = bf16's unit roundoff)
    statistics:                             the two formulas of test_convtranspose3d_epilogue_batchnorm_statistics, on the float64 fold
                                            of the partial rows against the sums over the STORED output; every row finite
"""
import functools
import json

import torch
import torch.nn.functional as F

F32_BAR = 1e-4
BF16_U = 2.0 ** -8

S2D_OK, S2D_ERR_UNSUPPORTED = 0, -2

# (key, cin, cout, (n, d, h, w)): the smallest shapes at which each branch of the dispatch can go wrong
SHAPES = [
    ("s01", 16, 3, (1, 1, 1, 8)),        # every neighbour is padding
    ("s02", 16, 3, (1, 2, 5, 64)),       # exactly one full x tile (CT_TX 64): the halo column x0 + 64 is outside; h = 5: a 1-row group of the 4-row blocks
    ("s03_co1", 16, 1, (2, 3, 4, 72)),   # a second x tile of 8 cells, halo from the neighbouring tile on both sides; z ring exactly full;
    ("s03_co2", 16, 2, (2, 3, 4, 72)),   # the channel masks of the (co, kx) column mapping and of the direct == 2 weight image
    ("s03_co3", 16, 3, (2, 3, 4, 72)),
    ("s03_co4", 16, 4, (2, 3, 4, 72)),
    ("s04", 16, 3, (1, 5, 9, 136)),      # three x tiles; the z ring wraps
    ("s05", 16, 3, (5, 5, 41, 8)),       # 1025 rows against the narrow cap of 1024: rows_per_block 2, 511 empty slabs
    ("s06", 16, 3, (2, 8, 1025, 8)),     # 16400 data-gradient items > 4096 blocks x 4 waves: the sweep loops; rows_per_block 17, ragged block, empty slabs
    ("s07a", 32, 3, (1, 2, 17, 72)),     # 32-channel narrow kernels (CIT 2, NT 2), fold included; h = 17: a ragged 1-row chunk of both tile maps
    ("s07b", 32, 3, (2, 1, 4, 8)),
    ("s08", 32, 32, (2, 2, 9, 72)),      # row-major weight gradient CIT 2; fp32 / bf16 data-gradient maps get different yc, both with a ragged last chunk
    ("s09", 32, 32, (1, 3, 43, 68)),     # 129 rows against the row-major cap of 128; w % 8 != 0
    ("s10", 16, 3, (1, 2, 3, 68)),       # cout <= 4 but not narrow: row-major CIT 1; the norm fold is refused
    ("s11a", 16, 6, (1, 2, 3, 24)),      # COP 8 without N4 (the channel-pair mapping)
    ("s11b", 32, 8, (1, 2, 3, 12)),
    ("s11c", 16, 16, (1, 2, 3, 132)),    # the nt 1 -> 2 boundary ...
    ("s11d", 16, 17, (1, 2, 3, 132)),    # ... with one live column in the second tile
    ("s12a", 32, 4, (1, 27, 19, 6)),     # w % 4 != 0: the MFMA weight-gradient kernels, 513 rows against their cap of 512; _d16 / _norm / _x16 refuse
    ("s12b", 16, 32, (1, 2, 3, 66)),
    ("s13", 32, 32, (1, 1, 18, 376)),    # full row width: ct_chunk_rows drops below 16 for the forward (8, 8, 2) and further for the data gradients
]
SHAPE = {k: (cin, cout, shp) for k, cin, cout, shp in SHAPES}
UNROUNDED = ["s03_co3", "s08", "s12a"]          # narrow, row-major and MFMA weight-gradient kernels; N4, COP 32 data gradients


# ---- what the dispatch is expected to do (a host restatement of the launchers' predicates and of ct_wgrad_blocks_for) ------------------
def expect_mfma(cin, cout):
    return cin in (16, 32) and 1 <= cout <= 32


def expect_narrow(cout, w):
    return cout <= 4 and w % 8 == 0


def expect_d16(cin, cout, shp):
    n, d, h, w = shp
    return expect_mfma(cin, cout) and cout * 8 * d * h * w * 4 < (1 << 31) and (expect_narrow(cout, w) or w % 4 == 0)


def expect_norm(cin, cout, shp):
    return expect_d16(cin, cout, shp) and expect_narrow(cout, shp[3])


def expect_x16(cin, cout, shp):
    return expect_norm(cin, cout, shp) and cin == 16


def wgrad_plan(cin, cout, shp):
    """-> dict(kind, blocks, rows_per_block, used, empty, last_rows, ws_bytes): the slabs the weight gradient writes and ct_slab_reduce sums"""
    n, d, h, w = shp
    rows = n * d * h
    kind, cap = ("narrow", 1024) if expect_narrow(cout, w) else ("rows", 128) if w % 4 == 0 else ("mfma", 512)
    bx = min(rows, cap)
    rpb = -(-rows // bx)
    used = -(-rows // rpb)
    return dict(kind=kind, blocks=bx, rows_per_block=rpb, used=used, empty=bx - used, last_rows=rows - (used - 1) * rpb,
                ws_bytes=-(-(bx * cin * cout * 64 * 4) // 256) * 256)


def dgrad_items(shp):
    n, d, h, w = shp
    return n * d * h * (-(-w // 64))


def chunk_rows(row_bytes, rows_per_y, halo, planes):
    yc = 16
    while yc > 1 and (rows_per_y * yc + halo) * planes * row_bytes > (2 << 20):
        yc >>= 1
    return yc


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def bf16r(t):
    """torch's rounding to bf16 (nearest even), widened back"""
    return t.to(torch.bfloat16).to(t.dtype)


def normalised(x, scale, shift):
    """relu(x * scale[ci] + shift[ci]) in float64 -> fp32; exact for the `rounded` inputs (asserted)"""
    v = torch.relu(x.double() * scale.double().view(1, -1, 1, 1, 1) + shift.double().view(1, -1, 1, 1, 1))
    v32 = v.float()
    assert torch.equal(v32.double(), v), "the norm-fold inputs must make x * scale + shift exact in fp32"
    return v32


def make_inputs(cin, cout, shp, rounded=True, seed=0):
    n, d, h, w = shp
    g = torch.Generator().manual_seed(1000 * cin + 31 * cout + 7 * w + h + seed)
    t = {}
    if rounded:
        t["x"] = torch.randint(-128, 129, (n, cin, d, h, w), generator=g).float() / 32
        t["w"] = bf16r(torch.randn(cin, cout, 4, 4, 4, generator=g) * 0.1)
        t["dout"] = bf16r(torch.randn(n, cout, 2 * d, 2 * h, 2 * w, generator=g))
    else:
        t["x"] = torch.randn(n, cin, d, h, w, generator=g)
        t["w"] = torch.randn(cin, cout, 4, 4, 4, generator=g) * 0.1
        t["dout"] = torch.randn(n, cout, 2 * d, 2 * h, 2 * w, generator=g)
    t["bias"] = torch.randn(cout, generator=g) * 0.5
    t["scale"] = torch.randint(4, 13, (cin,), generator=g).float() / 8
    shift = torch.randint(-8, 9, (cin,), generator=g).float() / 16
    shift[0::2] = shift[0::2].abs().clamp_min(1 / 16)   # half the channels: relu(shift) != 0
    t["shift"] = shift
    return t


def reference(x_op, w_op, bias, dout_op):
    """float64 conv_transpose3d(4, 2, 1) over the given operands -> (y, din, dW [cin][cout][4][4][4])"""
    x = x_op.double().requires_grad_(True)
    w = w_op.double().requires_grad_(True)
    y = F.conv_transpose3d(x, w, None if bias is None else bias.double(), stride=2, padding=1)
    din, dw = torch.autograd.grad(y, [x, w], dout_op.double())
    return y.detach(), din, dw


def reference_with_border(x_op, border, w_op, bias):
    """the forward over x_op with its padding cells holding border[ci] instead of zero (a zero border reproduces `reference`): the output
    a normalise-on-load kernel would give if it normalised the padding cells too"""
    n, c, d, h, w = x_op.shape
    xp = border.double().view(1, c, 1, 1, 1).expand(n, c, d + 2, h + 2, w + 2).clone()
    xp[:, :, 1:-1, 1:-1, 1:-1] = x_op.double()
    y = F.conv_transpose3d(xp, w_op.double(), None if bias is None else bias.double(), stride=2, padding=1)
    return y[:, :, 2:2 * d + 2, 2:2 * h + 2, 2:2 * w + 2].contiguous()   # padded cell h + 1 -> output o + 2


@functools.lru_cache(maxsize=None)
def case(key, rounded=True):
    """inputs and float64 references of one shape, computed once per process and shared (never modified) by every test that needs them:
    y / din / dw over the plain operands, yn / dwn over the normalised x operand (where the fold is supported)"""
    cin, cout, shp = SHAPE[key]
    t = make_inputs(cin, cout, shp, rounded)
    c = dict(t, key=key, cin=cin, cout=cout, shape=shp, rounded=rounded)
    c["y"], c["din"], c["dw"] = reference(bf16r(t["x"]), bf16r(t["w"]), t["bias"], bf16r(t["dout"]))
    if rounded:
        assert torch.equal(bf16r(t["x"]), t["x"]) and torch.equal(bf16r(t["dout"]), t["dout"])
        c["xn"] = normalised(t["x"], t["scale"], t["shift"])
        if expect_norm(cin, cout, shp):
            c["yn"], _, c["dwn"] = reference(bf16r(c["xn"]), bf16r(t["w"]), t["bias"], t["dout"])
    return c


# ---- the checks: measured, collected, printed, then asserted --------------------------------------------------------------------------
class Report:
    """the figures of one case.  Every check records (what, kind, value, bound, ok); assert_all() prints them all, then fails on the first
    that missed.  to_json / from_json carry them from a child process to the test that asserts them."""

    def __init__(self, items=None):
        self.items = list(items or [])

    def add(self, what, kind, value, bound, ok, detail=""):
        self.items.append(dict(what=what, kind=kind, value=float(value), bound=float(bound), ok=bool(ok), detail=str(detail)))
        return bool(ok)

    # fp32-stored result against float64
    def f32(self, what, got, ref):
        got = got.detach().cpu()
        if got.dtype != torch.float32 or tuple(got.shape) != tuple(ref.shape):
            return self.add(what, "f32", float("nan"), F32_BAR, False, f"dtype / shape {got.dtype} {tuple(got.shape)} vs {tuple(ref.shape)}")
        unwritten = int((~torch.isfinite(got)).sum())
        top = ref.abs().max().item()
        rel = (got.double() - ref).abs().max().item() / top if top > 0 else float("inf")
        return self.add(what, "f32", rel, F32_BAR, unwritten == 0 and rel <= F32_BAR, f"{unwritten} non-finite elements" if unwritten else "")

    # bf16-stored result against float64, elementwise
    def bf16(self, what, got, ref):
        got = got.detach().cpu()
        if got.dtype != torch.bfloat16 or tuple(got.shape) != tuple(ref.shape):
            return self.add(what, "bf16", float("nan"), 0.0, False, f"dtype / shape {got.dtype} {tuple(got.shape)} vs {tuple(ref.shape)}")
        unwritten = int((~torch.isfinite(got.float())).sum())
        top = ref.abs().max().item()
        err = (got.double() - ref).abs()
        excess = (err - (BF16_U * ref.abs() + F32_BAR * top)).max().item()   # <= 0: inside the bar everywhere
        rel = err.max().item() / top if top > 0 else float("inf")
        ok = unwritten == 0 and top > 0 and excess <= 0
        return self.add(what, "bf16", rel, BF16_U + F32_BAR, ok, f"{unwritten} non-finite; worst excess over the elementwise bar {excess:.3e}")

    # bit identity
    def same(self, what, a, b):
        a, b = a.detach().cpu(), b.detach().cpu()
        if a.dtype != b.dtype or a.shape != b.shape:
            return self.add(what, "equal", float("nan"), 0, False, f"{a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}")
        bits = torch.int16 if a.element_size() == 2 else torch.int32
        diff = int((a.contiguous().view(bits) != b.contiguous().view(bits)).sum())
        finite = bool(torch.isfinite(a.float()).all())
        return self.add(what, "equal", diff, 0, diff == 0 and finite, "" if finite else "non-finite elements")

    # epilogue statistics [tiles][2][cout] against the sums over the stored output
    def stats(self, what, partial, stored, tiles):
        partial, yd = partial.detach().cpu(), stored.detach().cpu().double()
        n, cout = yd.shape[0], yd.shape[1]
        if tuple(partial.shape) != (tiles, 2, cout):
            return self.add(what, "stats", float("nan"), 0, False, f"shape {tuple(partial.shape)} vs {(tiles, 2, cout)}")
        bad_rows = int((~torch.isfinite(partial).flatten(1).all(1)).sum())
        if bad_rows:
            return self.add(what, "stats", float("nan"), 0, False, f"{bad_rows} of {tiles} partial rows not finite (never written)")
        fold = partial.double().sum(0)
        s1, s2 = yd.sum(dim=(0, 2, 3, 4)), (yd ** 2).sum(dim=(0, 2, 3, 4))
        count = yd[0, 0].numel() * n
        b1, b2 = 1e-5 * s2.sqrt().max().item() * count ** 0.5, 1e-5 * s2.abs().max().item()
        e1, e2 = (fold[0] - s1).abs().max().item(), (fold[1] - s2).abs().max().item()
        ok1 = self.add(what + " sum", "stats", e1, b1, e1 <= b1)
        ok2 = self.add(what + " sum of squares", "stats", e2, b2, e2 <= b2)
        return ok1 and ok2

    # a return code
    def rc(self, what, got, want):
        return self.add(what, "rc", got, want, got == want)

    # a refused call left its poisoned outputs alone (buffers: uint8 views)
    def untouched(self, what, buffers, poison):
        changed = sum(int((b.detach().cpu().contiguous().view(torch.uint8) != poison).sum()) for b in buffers)
        return self.add(what, "untouched", changed, 0, changed == 0)

    # both guards of every allocation of a ws_guard.GuardLog hold
    def guards(self, what, log):
        try:
            log.check()
        except AssertionError as e:
            return self.add(what, "guards", 1, 0, False, e)
        return self.add(what, "guards", 0, 0, True)

    def failures(self):
        return [i for i in self.items if not i["ok"]]

    def assert_all(self, tag=""):
        for i in self.items:
            print(f"CT_CHECK {tag} | {i['what']} | {i['kind']} | {i['value']:.4e} | bound {i['bound']:.4e} | {'ok' if i['ok'] else 'FAIL'} {i['detail']}")
        bad = self.failures()
        assert self.items, f"{tag}: nothing was checked"
        assert not bad, f"{tag}: {len(bad)} of {len(self.items)} checks failed, first: {bad[0]}"

    def to_json(self):
        return json.dumps(self.items)

    @classmethod
    def from_json(cls, text):
        return cls(json.loads(text))


def host_partials(stored, tiles):
    """a correct [tiles][2][cout] statistics list for a stored output: per-chunk (sum, sum of squares), fp32 like the kernels write them"""
    n, cout = stored.shape[:2]
    flat = stored.double().transpose(0, 1).reshape(cout, -1)
    rows = [torch.stack([ch.sum(1), (ch ** 2).sum(1)]) for ch in torch.tensor_split(flat, tiles, dim=1)]
    return torch.stack(rows).float()

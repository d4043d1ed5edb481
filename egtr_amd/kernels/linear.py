"""Bindings of the linear-layer kernels (csrc/linear*.hip, gemm_split.hip, ffn_*.hip): the
skinny / grouped linears, the split-bf16 GEMM with its weight packers, the row-panel FFN / projection / encoder-tail
launches and the column sums.  No routing decisions here -- ``egtr_amd.ops`` decides and re-exports every name below."""
import torch

from .. import _lib
from .._lib import _chk
from .backbone import xs_bytes, xs_split
from .derived import cached_weights
from .elementwise import add_layer_norm_into

__all__ = ["ffn_layernorm_bf16", "linear_bf16", "column_sum", "weighted_column_sum", "linear_split_ex", "DeferredLayerNorm",
           "linear_grouped", "gemm_split_weights", "gemm_split_tile", "gemm_split_tile_pair", "gemm_split_tile_pairs",
           "linear_split_bf16_wgrad", "linear_split_bf16", "linear_split_bf16_grouped", "ffn_fused", "encoder_tail_fused",
           "proj_ln_fused", "proj_multi_fused"]


def _c16(t):
    """Contiguous AND 16-byte aligned (a contiguous view with an odd storage offset is copied): what the C entries'
    vector loads require; they answer EGTR_E_UNSUPPORTED otherwise."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def ffn_layernorm_bf16(x, fc1, fc2, ln, pos=None):
    """LayerNorm(x + fc2(relu(fc1(x)))) for a bf16 model in one launch (egtr_ffn_layernorm_bf16); with ``pos`` ([rows_p, 256]
    bf16, tiled over the rows) also returns the bf16 sum of the result and the position rows.  Inference only."""
    lib = _lib.lib()
    x2 = _chk(x.reshape(-1, 256).contiguous(), "x", torch.bfloat16)
    F_ = fc1.weight.shape[0]

    def pack():
        w1 = _chk(fc1.weight.detach().contiguous(), "fc1.weight", torch.bfloat16)
        w2 = _chk(fc2.weight.detach().contiguous(), "fc2.weight", torch.bfloat16)
        out = torch.empty(int(lib.egtr_ffn_packed_weights_bytes(F_)) // 2, dtype=torch.bfloat16, device=w1.device)
        _lib.launch("egtr_ffn_pack_weights_bf16", w1.data_ptr(), w2.data_ptr(), 256, F_, out.data_ptr())
        return out

    wpk = cached_weights(fc1, "ffn_bf16_packed", [fc1.weight, fc2.weight], pack)
    ts = [wpk] + [_chk(t.detach().contiguous(), n, torch.bfloat16)
                  for t, n in ((fc1.bias, "fc1.bias"), (fc2.bias, "fc2.bias"), (ln.weight, "ln.weight"), (ln.bias, "ln.bias"))]
    M = x2.shape[0]
    y = torch.empty_like(x2)
    yp = p2 = None
    prow = 1
    if pos is not None:
        p2 = _chk(pos.reshape(-1, 256).contiguous(), "pos", torch.bfloat16)
        prow = p2.shape[0]
        if M % prow != 0:
            raise ValueError("ffn_layernorm_bf16: pos must tile the rows")
        yp = torch.empty_like(x2)
    _lib.launch("egtr_ffn_layernorm_bf16", x2.data_ptr(), *[t.data_ptr() for t in ts], float(ln.eps), _lib.ptr(p2), prow,
                y.data_ptr(), _lib.ptr(yp), M, 256, fc1.weight.shape[0])
    y = y.view(x.shape)
    return y if pos is None else (y, yp.view(x.shape))


def linear_bf16(x, weight, bias=None, relu=False, alpha=1.0):
    """act(alpha (x . W^T + b)) for bf16 tensors (egtr_linear_bf16): fp32 accumulation, one rounding of the result.
    Inference only."""
    K, N = x.shape[-1], weight.shape[0]
    x2 = _chk(x.reshape(-1, K).contiguous(), "x", torch.bfloat16)
    w = _chk(weight.detach().contiguous(), "weight", torch.bfloat16)
    b = _chk(bias.detach().contiguous(), "bias", torch.bfloat16) if bias is not None else None
    if weight.shape[1] != K:
        raise ValueError("linear_bf16: weight must be [N, K]")
    M = x2.shape[0]
    if (x2.data_ptr() | w.data_ptr()) % 16 != 0:   # a view at an odd offset: the kernel's 16-byte operand loads need alignment
        y = torch.nn.functional.linear(x2, w, b)
        if alpha != 1.0:
            y = y * alpha
        return (torch.relu(y) if relu else y).view(*x.shape[:-1], N)
    y = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    if M > 0:
        _lib.launch("egtr_linear_bf16", x2.data_ptr(), K, w.data_ptr(), _lib.ptr(b), y.data_ptr(), N, M, N, K, 1 if relu else 0,
                    float(alpha))
    return y.view(*x.shape[:-1], N)


def column_sum(g, relu_output=None, inplace=False):
    """g [M, N] fp32 -> column sums [N] (the bias gradient of a linear layer), egtr_column_sum_f32: one launch for
    object-query-sized M.  With ``relu_output`` (the layer's post-ReLU output) returns (g * [y > 0], its column sums);
    ``inplace``: the masked gradient overwrites ``g`` (every element is read and written by the same thread)."""
    lib = _lib.lib()
    g = _chk(_c16(g), "grad", torch.float32)
    M, N = g.shape
    ws = torch.empty(int(lib.egtr_column_sum_workspace_floats(M, N)), dtype=torch.float32, device=g.device)
    out = torch.empty(N, dtype=torch.float32, device=g.device)
    gm = (g if inplace else torch.empty_like(g)) if relu_output is not None else None
    ro = _chk(_c16(relu_output), "relu_output", torch.float32) if gm is not None else None
    _lib.launch("egtr_column_sum_f32", g.data_ptr(), _lib.ptr(ro), _lib.ptr(gm), ws.data_ptr(), out.data_ptr(), M, N)
    return out if gm is None else (gm, out)


def weighted_column_sum(g, row_weight):
    """sum_r row_weight[r] * g[r, :] for g [M, N] fp32 (egtr_weighted_column_sum_f32)."""
    lib = _lib.lib()
    g = _chk(g.contiguous(), "g", torch.float32)
    w = _chk(row_weight.reshape(-1).contiguous(), "row_weight", torch.float32)
    M, N = g.shape
    if w.numel() != M:
        raise RuntimeError("weighted_column_sum: one weight per row expected")
    ws = torch.empty(int(lib.egtr_column_sum_workspace_floats(M, N)), dtype=torch.float32, device=g.device)
    out = torch.empty(N, dtype=torch.float32, device=g.device)
    _lib.launch("egtr_weighted_column_sum_f32", g.data_ptr(), w.data_ptr(), ws.data_ptr(), out.data_ptr(), M, N)
    return out


# ``terms``: which arithmetic a split-GEMM binding launches; it travels as the trailing argument of the C entries.  6 (the
# default everywhere): the six-term split-bf16 product, fp32 to the last bit, on the three-piece weight stream
# [N/128][K/32][3][128][32].  1: one product per element, each operand rounded once to bf16 (round to nearest even), fp32
# accumulation, on the one-piece stream [N/128][K/32][128][32]; ``egtr_amd.ops`` passes it from ``ops.matmul_precision()`` in
# its training Functions and nowhere else.
def _pieces(terms):
    if terms not in (1, 6):
        raise ValueError(f"terms must be 6 (split-bf16, fp32 accuracy) or 1 (operands rounded to bf16), got {terms!r}")
    return 3 if terms == 6 else 1


def _stream_shape(N, K, terms):
    return (N // 128, K // 32, 3, 128, 32) if _pieces(terms) == 3 else (N // 128, K // 32, 128, 32)


_EPILOGUE = frozenset(("row_keep", "relu_ref", "add1", "add2", "colpart"))


def _split_launch(who, problems, M, K, terms, x_as_given=False):
    """ONE launch of egtr_linear_split_bf16_ex_f32 for 1..16 problems (kMaxProblems of csrc/gemm_split.hip) of M rows and
    reduction length K, after the checks every split-GEMM binding shares.  A problem is a dict: x [..., K] (viewed as rows; copied
    when the kernel's stride / alignment rules ask for it), wt (tiled weight of ``terms``), N, and optionally b, relu, out (float32
    [M, N] view, unit inner stride, row stride % 4 == 0, 16-byte aligned base: rows of a larger buffer are fine), pos
    ([pos_rows, K], pos_rows divides M), row_keep, relu_ref, add1, add2, colpart.  ``x_as_given``: x is the [M, >= K] matrix
    itself (a column block of a wider buffer has more than K columns, which no row view expresses) and is never copied.
    Returns the outputs."""
    import ctypes
    n = len(problems)
    if not 0 < n <= 16:
        raise RuntimeError(f"{who}: 1..16 problems in one launch, got {n}")
    # One pass: a problem becomes its row of the ten host arrays.  The eager inference forward is host-bound and makes three
    # such launches per image, one of them with 14 problems, so nothing below looks at a problem twice.
    rows, ys, keep = [], [], []
    epi = None      # the training step's epilogue operands, key -> per-problem tensors; built once a problem names one
    for i, it in enumerate(problems):
        x2 = it["x"] if x_as_given else _lib.row_view(it["x"], K)
        N, wt = int(it["N"]), it["wt"]
        if not x2.is_cuda or x2.dtype != torch.float32 or x2.dim() != 2 or x2.stride(1) != 1:
            raise RuntimeError(f"{who}: x must be a float32 CUDA/HIP tensor with unit inner stride")
        if x2.shape[0] != M:
            raise RuntimeError(f"{who}: all inputs must have the same number of rows")
        _chk(wt, "wt", torch.bfloat16)
        if tuple(wt.shape) != _stream_shape(N, K, terms):
            raise RuntimeError(f"{who}: wt must be {list(_stream_shape(N, K, terms))} for terms={terms}, got {tuple(wt.shape)}")
        b = it.get("b")
        if b is not None:
            b = _chk(b.detach().contiguous(), "bias", torch.float32)
        y = it.get("out")
        if y is None:
            y = torch.empty(M, N, dtype=torch.float32, device=x2.device)
        elif not (y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and tuple(y.shape) == (M, N)
                  and y.stride(1) == 1 and y.stride(0) % 4 == 0 and y.data_ptr() % 16 == 0):
            raise RuntimeError(f"{who}: out must be a float32 [rows, N] view with unit inner stride, a row stride that is a "
                               "multiple of 4 and a 16-byte aligned base")
        pos = it.get("pos")
        if pos is not None:
            pos = _chk(pos.reshape(-1, K).contiguous(), "pos", torch.float32)
            if M % pos.shape[0]:
                raise RuntimeError(f"{who}: pos must tile the rows")
        if not _EPILOGUE.isdisjoint(it):
            if epi is None:
                epi = {key: [None] * n for key in _EPILOGUE}
            for key in _EPILOGUE:
                epi[key][i] = it.get(key)
        # x, ldx, w_tiled, bias, y, ldy, N, relu, pos, pos_rows: the order of the C entry's arrays
        rows.append((x2.data_ptr(), x2.stride(0), wt.data_ptr(), _lib.ptr(b), y.data_ptr(), y.stride(0), N,
                     1 if it.get("relu") else 0, _lib.ptr(pos), pos.shape[0] if pos is not None else 1))
        ys.append(y)
        keep.append((x2, b, pos))      # (possibly copies: alive until the launch is queued)
    PA, IA = ctypes.c_void_p * n, ctypes.c_int * n
    px, ldx, pw, pb, py, ldy, Ns, relu, ppos, prows = zip(*rows)
    tail = (None,) * 7      # an option no problem uses travels as a NULL array
    if epi is not None:
        rr, a1, a2 = epi["relu_ref"], epi["add1"], epi["add2"]
        for key, ts in (("relu_ref", rr), ("add1", a1), ("add2", a2)):
            for t in ts:
                if t is not None and (t.stride(-1) != 1 or t.dtype != torch.float32 or not t.is_cuda):
                    raise RuntimeError(f"{who}: {key} must be a float32 device tensor with unit inner stride")
        if any(p is not None and q is not None and p.stride(0) != q.stride(0) for p, q in zip(a1, a2)):
            raise RuntimeError(f"{who}: add1 and add2 must share their row stride")

        def ptrs(ts):
            return PA(*[_lib.ptr(t) for t in ts]) if any(t is not None for t in ts) else None

        def lds(ts):
            return IA(*[(t.stride(0) if t is not None else 0) for t in ts])

        tail = (ptrs(epi["row_keep"]), ptrs(rr), lds(rr), ptrs(a1), ptrs(a2),
                lds([p if p is not None else q for p, q in zip(a1, a2)]), ptrs(epi["colpart"]))
    _lib.launch("egtr_linear_split_bf16_ex_f32", n, PA(*px), IA(*ldx), PA(*pw), PA(*pb), PA(*py), IA(*ldy), IA(*Ns), IA(*relu),
                M, K, PA(*ppos), IA(*prows), *tail, terms)
    return ys


def linear_split_ex(problems, M, K, terms=6):
    """Up to 16 token-sized linears with the same M and K in one launch of the split-bf16 GEMM with the training step's epilogue
    options (egtr_linear_split_bf16_ex_f32).  ``problems``: dicts with x [M, >=K] (unit inner stride), wt (tiled weight), N,
    and optionally b, relu, out ([M, N] view with unit inner stride), pos ([pos_rows, K], pos_rows divides M), row_keep ([M]
    uint8), relu_ref
    ([M, N]), add1 / add2 ([M, N], may alias out), colpart ([ceil(M / 32), N]).  Returns the outputs.  No autograd.
    ``terms=1``: the one-term arithmetic on one-piece weight streams."""
    return _split_launch("linear_split_ex", problems, int(M), int(K), terms, x_as_given=True)


def _wgrad_ex(g, x, x_pos=None, row_keep=None, terms=6):
    """g [M, N]^T . (x [+ x_pos rows]) [M, K] -> [N, K] with optional row mask on g (egtr_linear_split_bf16_wgrad_ex_f32)."""
    lib = _lib.lib()
    M, N = g.shape
    K = x.shape[1]
    _pieces(terms)
    ws = torch.empty(int(lib.egtr_linear_split_bf16_wgrad_workspace_floats(M, N, K, terms)), dtype=torch.float32, device=g.device)
    gw = torch.empty(N, K, dtype=torch.float32, device=g.device)
    _lib.launch("egtr_linear_split_bf16_wgrad_ex_f32", g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), gw.data_ptr(),
                ws.data_ptr(), M, N, K, _lib.ptr(x_pos), x_pos.shape[0] if x_pos is not None else 1, _lib.ptr(row_keep), terms)
    return gw


def _skinny_fwd(x2, w, b, alpha=1.0, relu=False):
    """act((x W^T + b) * alpha) for object-query rows (egtr_linear_f32), plain tensors, no autograd."""
    M, K = x2.shape
    N = w.shape[0]
    y = torch.empty(M, N, dtype=torch.float32, device=x2.device)
    _lib.launch("egtr_linear_f32", x2.data_ptr(), w.data_ptr(), _lib.ptr(b), y.data_ptr(), M, K, N, float(alpha),
                1 if relu else 0)
    return y


def _skinny_bwd(g, x2, w, alpha=1.0, relu_out=None, want_gb=True, add1=None, add2=None, out=None):
    """(grad_x [+ add1 + add2], grad_w, grad_b) of ``_skinny_fwd`` in one launch (egtr_linear_backward_acc_f32)."""
    M, N = g.shape
    K = w.shape[1]
    gx = out if out is not None else torch.empty(M, K, dtype=torch.float32, device=g.device)
    gw = torch.empty(N, K, dtype=torch.float32, device=g.device)
    gb = torch.empty(N, dtype=torch.float32, device=g.device) if want_gb else None
    _lib.launch("egtr_linear_backward_acc_f32", g.data_ptr(), _lib.ptr(relu_out), x2.data_ptr(), w.data_ptr(), float(alpha),
                gx.data_ptr(), gw.data_ptr(), _lib.ptr(gb), M, K, N, _lib.ptr(add1), _lib.ptr(add2))
    return gx, gw, gb


class DeferredLayerNorm:
    """y = LayerNorm(a + b) that has NOT been computed yet: the skinny linears that consume y apply it as a prologue
    (``linear_grouped`` items with ``x=<DeferredLayerNorm>``; egtr_linear_grouped_ln_f32) and the first such launch also
    stores y into ``.out``.  Replaces the decoder's stand-alone residual-add + LayerNorm launches (4.8 us each at 200 rows:
    launch floor) at inference.  ``materialize()`` runs the stand-alone kernel when no linear consumes y."""

    def __init__(self, a, b, ln, out=None):
        if a.shape != b.shape or a.shape[-1] != 256:
            raise ValueError("DeferredLayerNorm: two [.., 256] tensors")
        self.a, self.b, self.ln = a, b, ln
        self.out = out if out is not None else torch.empty_like(a)
        self.done = False        # .out holds y
        self.claimed = False     # a group of a launch being assembled will store y

    @property
    def shape(self):
        return self.a.shape

    @property
    def device(self):
        return self.a.device

    def materialize(self):
        if not self.done:
            add_layer_norm_into(self.a, self.b, self.ln, self.out)
            self.done = self.claimed = True
        return self.out


def linear_grouped(items):
    """Several independent skinny linears in ONE HIP launch (egtr_linear_grouped_ln_f32).  ``items`` is a list of dicts:
    x [.., K] (or a ``DeferredLayerNorm``: the LayerNorm runs as the layer's prologue, K = 256), w [N, K], b [N] or None,
    optional pos ([pos_rows, 256], added to a DeferredLayerNorm input after the LayerNorm), out (2-D view [rows, N] with
    unit inner stride: rows of a larger buffer), alpha_x (scale on x), alpha (scale after the bias), relu.  Returns the
    list of outputs ([.., N], or the given ``out`` views).  Inference only (no autograd)."""
    import ctypes
    G = len(items)
    if not 0 < G <= 16:
        raise ValueError("linear_grouped: 1..16 groups")
    x0 = items[0]["x"]
    K = x0.shape[-1]
    xs, ws, bs, ys, Ms, Ns, lds, ax, al, rl, outs, keep = [], [], [], [], [], [], [], [], [], [], [], []
    lres, lga, lbe, leps, lpos, lprows, lout = [], [], [], [], [], [], []
    any_ln = False
    for it in items:
        x, w, b = it["x"], it["w"], it.get("b")
        dln = x if isinstance(x, DeferredLayerNorm) else None
        if dln is not None and dln.done:
            x, dln = dln.out, None
        lead = tuple(x.shape[:-1])
        if dln is not None:
            any_ln = True
            x2 = _chk(dln.a.reshape(-1, K).contiguous(), "x", torch.float32)
            r2 = _chk(dln.b.reshape(-1, K).contiguous(), "residual", torch.float32)
            ga = _chk(dln.ln.weight.detach().contiguous(), "ln.weight", torch.float32)
            be = _chk(dln.ln.bias.detach().contiguous(), "ln.bias", torch.float32)
            pos = it.get("pos")
            p2 = _chk(pos.reshape(-1, K).contiguous(), "pos", torch.float32) if pos is not None else None
            first = not dln.claimed     # exactly one group of the launch stores the LayerNorm result
            dln.claimed = True
            o2 = _chk(dln.out.view(-1, K), "ln_out", torch.float32) if first else None
            keep += [r2, ga, be, p2, o2]
            lres.append(r2.data_ptr()); lga.append(ga.data_ptr()); lbe.append(be.data_ptr()); leps.append(float(dln.ln.eps))
            lpos.append(_lib.ptr(p2)); lprows.append(p2.shape[0] if p2 is not None else 1)
            lout.append(_lib.ptr(o2))
        else:
            if it.get("pos") is not None:
                raise ValueError("linear_grouped: pos needs a DeferredLayerNorm input")
            x2 = _chk(x.reshape(-1, K).contiguous(), "x", torch.float32)
            lres.append(None); lga.append(None); lbe.append(None); leps.append(0.0); lpos.append(None); lprows.append(1)
            lout.append(None)
        w2 = _chk(w.detach().contiguous(), "w", torch.float32)
        b2 = _chk(b.detach().contiguous(), "b", torch.float32) if b is not None else None
        if w2.shape[1] != K or x.shape[-1] != K:
            raise ValueError("linear_grouped: all groups share K")
        M, N = x2.shape[0], w2.shape[0]
        out = it.get("out")
        if out is None:
            y2 = torch.empty(M, N, dtype=torch.float32, device=x2.device)
            outs.append(y2.view(*lead, N))
        else:
            if out.dim() != 2 or out.shape != (M, N) or out.stride(1) != 1:
                raise ValueError("linear_grouped: out must be a [rows, N] view with unit inner stride")
            y2 = out
            outs.append(out)
        keep += [x2, w2, b2, y2]
        xs.append(x2.data_ptr()); ws.append(w2.data_ptr()); bs.append(_lib.ptr(b2))
        ys.append(y2.data_ptr()); Ms.append(M); Ns.append(N); lds.append(y2.stride(0))
        ax.append(float(it.get("alpha_x", 1.0))); al.append(float(it.get("alpha", 1.0)))
        rl.append(1 if it.get("relu") else 0)
    PA, IA, FA = ctypes.c_void_p * G, ctypes.c_int * G, ctypes.c_float * G
    if any_ln:
        _lib.launch("egtr_linear_grouped_ln_f32", G, PA(*xs), PA(*ws), PA(*bs), PA(*ys), IA(*Ms), IA(*Ns), IA(*lds), FA(*ax),
                    FA(*al), IA(*rl), K, PA(*lres), PA(*lga), PA(*lbe), FA(*leps), PA(*lpos), IA(*lprows), PA(*lout))
        for it in items:
            if isinstance(it["x"], DeferredLayerNorm):
                it["x"].done = True
    else:
        _lib.launch("egtr_linear_grouped_f32", G, PA(*xs), PA(*ws), PA(*bs), PA(*ys), IA(*Ms), IA(*Ns), IA(*lds), FA(*ax),
                    FA(*al), IA(*rl), K)
    return outs


def gemm_split_weights(weight, terms=6):
    """W [N, K] fp32 -> the operand stream of gemm_split_bf16_f32: [N/128][K/32][3 pieces][128][32] bf16.  ``terms=1``: the
    one-piece stream of the one-term kernels, [N/128][K/32][128][32]: every element rounded once to bf16 (nearest even)."""
    N, K = weight.shape
    if _pieces(terms) == 1:
        return weight.detach().float().to(torch.bfloat16).view(N // 128, 128, K // 32, 32).permute(0, 2, 1, 3).contiguous()
    p = _split3_bf16(weight).view(3, N // 128, 128, K // 32, 32)
    return p.permute(1, 3, 0, 2, 4).contiguous()


def gemm_split_tile(weight, transposed=False, terms=6):
    """``gemm_split_weights(weight, terms)`` (``transposed``: of ``weight.t()``) in one launch (egtr_gemm_split_tile_weights_f32):
    the training step re-tiles each weight after every optimizer step, for the forward (W) and the data gradient (W^T)."""
    w = weight.detach()
    if not w.is_cuda or w.dtype != torch.float32 or w.dim() != 2 or w.stride(1) != 1:
        raise RuntimeError("gemm_split_tile: weight must be a 2-d float32 CUDA/HIP tensor with unit inner stride")
    N, K = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
    out = torch.empty(_stream_shape(N, K, terms), dtype=torch.bfloat16, device=w.device)
    _lib.launch("egtr_gemm_split_tile_weights_f32", w.data_ptr(), w.stride(0), 1 if transposed else 0, N, K, out.data_ptr(), terms)
    return out


def gemm_split_tile_pair(weight, terms=6):
    """(tiling of W, tiling of W^T) in one launch (egtr_gemm_split_tile_weights_pair_f32); N, K % 128 == 0."""
    w = weight.detach()
    if not w.is_cuda or w.dtype != torch.float32 or w.dim() != 2 or w.stride(1) != 1:
        raise RuntimeError("gemm_split_tile_pair: weight must be a 2-d float32 CUDA/HIP tensor with unit inner stride")
    N, K = w.shape
    out = torch.empty(2, _pieces(terms) * N * K, dtype=torch.bfloat16, device=w.device)
    _lib.launch("egtr_gemm_split_tile_weights_pair_f32", w.data_ptr(), w.stride(0), N, K, out.data_ptr(), terms)
    return out[0].view(_stream_shape(N, K, terms)), out[1].view(_stream_shape(K, N, terms))


def gemm_split_tile_pairs(weights, terms=6):
    """[(tiling of W, tiling of W^T)] for up to 8 weights in ONE launch (egtr_gemm_split_tile_weights_multi_f32).  An entry
    is a [N, K] tensor or a pair (w_a, w_b) of tensors with the same K: the row-wise concatenation [w_a; w_b] tiled as one
    weight without materialising it.  N, K multiples of 128."""
    import ctypes
    n = len(weights)
    P, I = ctypes.c_void_p, ctypes.c_int
    w1, w2, ld1, ld2, split, Ns, Ks, outs = [], [], [], [], [], [], [], []
    for e in weights:
        a, b = (e if isinstance(e, (tuple, list)) else (e, None))
        a = a.detach()
        b = b.detach() if b is not None else None
        for t in (a, b):
            if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1):
                raise RuntimeError("gemm_split_tile_pairs: 2-d float32 device tensors with unit inner stride expected")
        N, K = a.shape[0] + (b.shape[0] if b is not None else 0), a.shape[1]
        if b is not None and b.shape[1] != K:
            raise RuntimeError("gemm_split_tile_pairs: concatenated weights must share K")
        out = torch.empty(2, _pieces(terms) * N * K, dtype=torch.bfloat16, device=a.device)
        w1.append(a.data_ptr()); ld1.append(a.stride(0)); split.append(a.shape[0])
        w2.append(_lib.ptr(b)); ld2.append(b.stride(0) if b is not None else 0)
        Ns.append(N); Ks.append(K); outs.append(out)
    _lib.launch("egtr_gemm_split_tile_weights_multi_f32", n, (P * n)(*w1), (I * n)(*ld1), (P * n)(*w2), (I * n)(*ld2),
                (I * n)(*split), (I * n)(*Ns), (I * n)(*Ks), (P * n)(*[o.data_ptr() for o in outs]), terms)
    return [(o[0].view(_stream_shape(N, K, terms)), o[1].view(_stream_shape(K, N, terms))) for o, N, K in zip(outs, Ns, Ks)]


def linear_split_bf16_wgrad(g, x, terms=6):
    """g [M, N]^T . x [M, K] -> [N, K] (the weight gradient of a token-sized linear layer) through
    egtr_linear_split_bf16_wgrad_ex_f32 without its options; unit inner strides, N, K % 128 == 0."""
    if x.shape[0] != g.shape[0] or g.stride(1) != 1 or x.stride(1) != 1:
        raise RuntimeError("linear_split_bf16_wgrad: g [M, N] and x [M, K] with unit inner strides expected")
    return _wgrad_ex(g, x, terms=terms)


def linear_split_bf16(x, w_tiled, bias, N, relu=False, out=None, terms=6):
    """act(x W^T + b) through egtr_linear_split_bf16_f32 (no autograd).  x [..., K] fp32 with unit inner stride and a
    uniform row stride (a column block of a wider buffer is fine); w_tiled from ``gemm_split_weights``; ``out``: optional
    contiguous [rows, N] fp32 destination.  ``terms=1``: the one-term arithmetic on the one-piece stream
    (egtr_linear_split_bf16_ex_f32 with one problem)."""
    K = x.shape[-1]
    x2 = _lib.row_view(x, K)
    _chk(w_tiled, "w_tiled", torch.bfloat16)
    if tuple(w_tiled.shape) != _stream_shape(N, K, terms):
        raise RuntimeError(f"w_tiled must be {list(_stream_shape(N, K, terms))} for terms={terms}, got {tuple(w_tiled.shape)}")
    b = _chk(bias.detach().contiguous(), "bias", torch.float32) if bias is not None else None
    if out is not None:
        y = _chk(out, "out", torch.float32)
        if tuple(y.shape) != (x2.shape[0], N):
            raise RuntimeError(f"out must be [{x2.shape[0]}, {N}], got {tuple(y.shape)}")
    else:
        y = torch.empty(x2.shape[0], N, dtype=torch.float32, device=x.device)
    if _pieces(terms) == 1:
        _split_launch("linear_split_bf16", [dict(x=x2, wt=w_tiled, N=N, b=b, relu=relu, out=y)], x2.shape[0], K, 1)
    else:
        _lib.launch("egtr_linear_split_bf16_f32", x2.data_ptr(), x2.stride(0), w_tiled.data_ptr(), _lib.ptr(b), y.data_ptr(), N,
                    x2.shape[0], K, N, 1 if relu else 0)
    return y if out is not None else y.view(*x.shape[:-1], N)


def linear_split_bf16_grouped(items):
    """Several token-sized linears with the same row count and K in ONE launch (egtr_linear_split_bf16_ex_f32, six terms).
    ``items``: dicts with x [..., K], wt (from ``gemm_split_weights``), N, optional b, relu, out ([rows, N] view with unit inner
    stride: rows of a larger buffer are fine), pos ([pos_rows, K], added to x's rows (row % pos_rows) on the way into the
    kernel).  Returns the outputs ([rows, N]).  Inference only."""
    x0 = items[0]["x"]
    return _split_launch("linear_split_bf16_grouped", items, x0.numel() // x0.shape[-1], x0.shape[-1], 6)


def ffn_fused(x, fc1, fc2, ln=None, pos=None):
    """LayerNorm(x + fc2(relu(fc1(x)))) [and that + pos] in ONE HIP launch (egtr_ffn_x6_f32; reference:
    model/deformable_detr.py:1335-1345 in eval mode); without ``ln``: fc2(relu(fc1(x))).  The [rows, ffn_dim] hidden
    activation never leaves the compute units.  Returns y or (y, y + pos).  Inference only."""
    K = x.shape[-1]
    x2 = _lib.row_view(x, K)
    rows, F = x2.shape[0], fc1.weight.shape[0]
    w1 = cached_weights(fc1, "xs_weight", [fc1.weight], lambda: xs_split(fc1.weight, weights=True))
    w2 = cached_weights(fc2, "xs_weight", [fc2.weight], lambda: xs_split(fc2.weight, weights=True))
    b1 = _chk(fc1.bias.detach().contiguous(), "fc1.bias", torch.float32)
    b2 = _chk(fc2.bias.detach().contiguous(), "fc2.bias", torch.float32)
    y = torch.empty(rows, K, dtype=torch.float32, device=x.device)
    g = bt = p2 = yp = None
    eps = 0.0
    if ln is not None:
        g = _chk(ln.weight.detach().contiguous(), "ln.weight", torch.float32)
        bt = _chk(ln.bias.detach().contiguous(), "ln.bias", torch.float32)
        eps = float(ln.eps)
        if pos is not None:
            p2 = _chk(pos.reshape(-1, K).contiguous(), "pos", torch.float32)
            if rows % p2.shape[0]:
                raise ValueError("ffn_fused: pos must tile the rows")
            yp = torch.empty_like(y)
    _lib.launch("egtr_ffn_x6_f32", x2.data_ptr(), x2.stride(0), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                _lib.ptr(g), _lib.ptr(bt), eps, _lib.ptr(p2), p2.shape[0] if p2 is not None else 0, y.data_ptr(), _lib.ptr(yp),
                rows, K, F)
    y = y.view(x.shape)
    return y if yp is None else (y, yp.view(x.shape))


def encoder_tail_fused(context, hidden, out_proj, ln1, fc1, fc2, ln2, pos=None):
    """ln2(y1 + fc2(relu(fc1(y1)))) with y1 = ln1(hidden + out_proj(context)) [and the result + pos] in ONE HIP launch
    (egtr_encoder_tail_x6_f32; reference: model/deformable_detr.py:1102, 1326-1345 in eval mode).  ``context``: the
    deformable attention's output before its output projection.  Returns y or (y, y + pos).  Inference only."""
    K = context.shape[-1]
    c2, h2 = _lib.row_view(context, K), _lib.row_view(hidden, K)
    rows, F = c2.shape[0], fc1.weight.shape[0]
    if h2.shape[0] != rows:
        raise ValueError("encoder_tail_fused: context and hidden must have the same rows")
    wp = cached_weights(out_proj, "xs_weight", [out_proj.weight], lambda: xs_split(out_proj.weight, weights=True))
    w1 = cached_weights(fc1, "xs_weight", [fc1.weight], lambda: xs_split(fc1.weight, weights=True))
    w2 = cached_weights(fc2, "xs_weight", [fc2.weight], lambda: xs_split(fc2.weight, weights=True))
    f32 = [_chk(t.detach().contiguous(), n, torch.float32)
           for t, n in ((out_proj.bias, "out_proj.bias"), (ln1.weight, "ln1.weight"), (ln1.bias, "ln1.bias"),
                        (fc1.bias, "fc1.bias"), (fc2.bias, "fc2.bias"), (ln2.weight, "ln2.weight"), (ln2.bias, "ln2.bias"))]
    bp, g1, be1, b1, b2, g2, be2 = f32
    y = torch.empty(rows, K, dtype=torch.float32, device=context.device)
    p2 = yp = None
    if pos is not None:
        p2 = _chk(pos.reshape(-1, K).contiguous(), "pos", torch.float32)
        if rows % p2.shape[0]:
            raise ValueError("encoder_tail_fused: pos must tile the rows")
        yp = torch.empty_like(y)
    _lib.launch("egtr_encoder_tail_x6_f32", c2.data_ptr(), c2.stride(0), h2.data_ptr(), h2.stride(0), wp.data_ptr(),
                bp.data_ptr(), g1.data_ptr(), be1.data_ptr(), float(ln1.eps), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(),
                b2.data_ptr(), g2.data_ptr(), be2.data_ptr(), float(ln2.eps), _lib.ptr(p2),
                p2.shape[0] if p2 is not None else 0, y.data_ptr(), _lib.ptr(yp), rows, K, F)
    y = y.view(hidden.shape)
    return y if yp is None else (y, yp.view(hidden.shape))


def proj_ln_fused(x, lin, residual=None, ln=None, pos=None):
    """LayerNorm(residual + lin(x)) [and that + pos] for a 256 -> 256 nn.Linear in ONE HIP launch (egtr_proj_ln_x6_f32;
    reference: the attention output projection + residual + LayerNorm, model/deformable_detr.py:1102, 1326-1330); without
    ``ln``: lin(x).  Returns y or (y, y + pos).  Inference only."""
    K = x.shape[-1]
    x2 = _lib.row_view(x, K)
    rows = x2.shape[0]
    w = cached_weights(lin, "xs_weight", [lin.weight], lambda: xs_split(lin.weight, weights=True))
    b = _chk(lin.bias.detach().contiguous(), "bias", torch.float32)
    y = torch.empty(rows, K, dtype=torch.float32, device=x.device)
    g = bt = p2 = yp = r2 = None
    eps = 0.0
    if ln is not None:
        r2 = _lib.row_view(residual, K)
        g = _chk(ln.weight.detach().contiguous(), "ln.weight", torch.float32)
        bt = _chk(ln.bias.detach().contiguous(), "ln.bias", torch.float32)
        eps = float(ln.eps)
        if pos is not None:
            p2 = _chk(pos.reshape(-1, K).contiguous(), "pos", torch.float32)
            yp = torch.empty_like(y)
    _lib.launch("egtr_proj_ln_x6_f32", x2.data_ptr(), x2.stride(0), w.data_ptr(), b.data_ptr(), _lib.ptr(r2),
                r2.stride(0) if r2 is not None else 0, _lib.ptr(g), _lib.ptr(bt), eps, _lib.ptr(p2),
                p2.shape[0] if p2 is not None else 0, y.data_ptr(), _lib.ptr(yp), rows, K)
    y = y.view(x.shape)
    return y if yp is None else (y, yp.view(x.shape))


def proj_multi_fused(x, w_xs, num_weights, bias=None):
    """out[w] = x @ W_w^T (+ bias_w) for ``num_weights`` stacked 256 -> 256 weights applied to the same rows, ONE launch
    (egtr_proj_multi_x6_f32): ``w_xs`` = ``xs_split(torch.cat(weights, 0), weights=True)``.  Returns [num_weights, rows, 256].
    Inference only."""
    K = x.shape[-1]
    x2 = _lib.row_view(x, K)
    rows = x2.shape[0]
    _chk(w_xs, "w_xs", torch.uint8)
    if w_xs.numel() != xs_bytes(num_weights * 256, 256):
        raise RuntimeError("proj_multi_fused: w_xs does not have the XS size of [num_weights * 256, 256]")
    b = _chk(bias.detach().contiguous(), "bias", torch.float32) if bias is not None else None
    out = torch.empty(num_weights, rows, K, dtype=torch.float32, device=x.device)
    _lib.launch("egtr_proj_multi_x6_f32", x2.data_ptr(), x2.stride(0), w_xs.data_ptr(), _lib.ptr(b), out.data_ptr(), rows, K,
                num_weights)
    return out


def _split3_bf16(w):
    """fp32 tensor -> [3, ...] bf16 pieces hi / mid / lo with hi + mid + lo == w to fp32 precision (round-to-nearest
    pieces; the residuals w - hi and (w - hi) - mid are exact in fp32)."""
    w = w.detach().float()
    hi = w.to(torch.bfloat16)
    r = w - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo])

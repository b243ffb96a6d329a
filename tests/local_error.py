"""TEST INFRASTRUCTURE: an fp64 reference with a DERIVED error bound per element, for every op family of the C ABI.

The global metric of the kernel tests (``||got - want||_2 / ||want||_2`` over the whole tensor) spends two thirds of its budget on
the one correct bf16 rounding of the output and spreads the rest over every element: a fault confined to one row, one tile edge or
one 16-byte store disappears in it (tests/test_local_error.py injects such faults and shows the global metric passing).  Here every
element is compared with the fp64 result of the same stored inputs (bf16 / h16 / fp32 values are exact in fp64) against a bound of
its own, built from unit roundoffs only:

  * the output's storage format: bf16 2^-8; fp32 2^-24; h16 (an IEEE half holding x * 2^-6) 2^-11 relative + 2^-18 absolute (its
    subnormal range);
  * the fp32 accumulator: u32 = 2^-24, times the number of operations of the op (K, the row length, ...) and the magnitude of what
    was summed (|A| |W|^T, not |A W^T|: cancellation does not shrink the rounding errors).

The bound an op family uses is written out in its ``*_reference`` function.  No bound has a constant fitted to a kernel's output;
there is no "allowed fraction of outliers" either -- one element over its bound fails.  ``store_bound`` applies the output roundoff
to ``|want| + accumulated error`` (the value that is rounded is the computed one, not the exact one).

Entry points: ``<family>_reference(...) -> (want, bound)`` in fp64, and ``check_<family>(got, ...)`` which asserts and returns the
worst ``|got - want| / bound``.  A failure names the worst element, its index modulo 256 / 128 / 16 (tile and fragment patterns can
be read off) and the worst row-relative error.  Every call prints its worst ratio; with SVR_LOCAL_ERROR_LOG=<file> it is appended
there as ``<test id>\\t<name>\\t<ratio>`` (profiles/local_error_headroom.txt is made from such a log -- a record, never an input to
a tolerance)."""
import dataclasses
import os

import torch
import torch.nn.functional as F

from ops_reference import (H16, H16_SCALE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_SILU, EPI_RESID_GATE, EPI_SWIGLU,
                           gemm_acc, gemm_bias_rows, gemm_place)

F64 = torch.float64
U32 = 2.0 ** -24                      # fp32 accumulator / arithmetic
U_BF16 = 2.0 ** -8                    # round-to-nearest into 8 significant bits: half an ulp is at most 2^-8 of the value
U_H16, ABS_H16 = 2.0 ** -11, 2.0 ** -18
LIP_SILU, LIP_GELU = 1.1, 1.13        # Lipschitz constants of SiLU (max |silu'| = 1.0998) and tanh-GELU (max |gelu'| = 1.129)
APPROX = 8 * U32                      # fast_exp2 / v_rcp_f32 in an activation or a softmax (1 ulp each, and the operations between them)
GN_ROWS_PER_BLOCK = 2048              # csrc/svr_elementwise.hip


def values(t):
    """stored tensor -> the fp64 values it stands for (h16: the half holds x * 2^-6)"""
    return t.to(F64) * (1.0 / H16_SCALE) if t.dtype == H16 else t.to(F64)


def out_roundoff(dtype):
    """(relative, absolute) roundoff of one store in ``dtype``"""
    if dtype == torch.bfloat16:
        return U_BF16, 0.0
    if dtype == H16:
        return U_H16, ABS_H16
    if dtype == torch.float32:
        return U32, 0.0
    if dtype == F64:
        return 0.0, 0.0
    raise ValueError(f"no storage format {dtype}")


def store_bound(want, acc_bound, dtype):
    """|stored - want| <= acc_bound + u_out * (|want| + acc_bound) + a_out: the computed value is within acc_bound of want, and
    the store rounds the computed value."""
    rel, ab = out_roundoff(dtype)
    return acc_bound + rel * (want.abs() + acc_bound) + ab


# ------------------------------------------------------------------------------------------------ the check itself
_worst_by_test = {}


def _test_id():
    return os.environ.get("PYTEST_CURRENT_TEST", "-").split(" ")[0]


def _record(name, worst):
    tid = _test_id()
    _worst_by_test[tid] = max(_worst_by_test.get(tid, 0.0), worst)
    print(f"[local_error] {name}: worst err/bound {worst:.3f}")
    log = os.environ.get("SVR_LOCAL_ERROR_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{tid}\t{name}\t{worst:.4f}\n")


def _mods(i):
    return f"{i} (mod 256: {i % 256}, mod 128: {i % 128}, mod 16: {i % 16})"


def worst_ratio(got, want, bound, mask=None):
    """max over the (masked) elements of |got - want| / bound, 0 where both vanish, inf where got is not finite or the bound is 0
    and the element differs; and the ratio tensor."""
    err = (values(got).reshape(want.shape) - want).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    if mask is not None:
        ratio = torch.where(mask, ratio, torch.zeros_like(ratio))
    return (float(ratio.max()) if ratio.numel() else 0.0), ratio


def check(name, got, want, bound, mask=None, before=None):
    """Assert |got - want| <= bound on every element (of ``mask``).  ``before``: the output tensor as it was before the launch --
    the elements outside ``mask`` must still hold those bits.  -> worst err / bound."""
    worst, ratio = worst_ratio(got, want, bound, mask)
    _record(name, worst)
    if mask is not None and before is not None:
        raw = torch.int16 if got.element_size() == 2 else torch.int32
        stray = (got.view(raw) != before.view(raw)) & ~mask
        assert not bool(stray.any()), f"{name}: the launch wrote {int(stray.sum())} elements that are not its own"
    if worst <= 1.0:
        return worst
    cols = want.shape[-1]
    flat = int(ratio.reshape(-1).argmax())
    r, c = divmod(flat, cols)
    g2, w2 = values(got).reshape(-1, cols), want.reshape(-1, cols)
    m2 = mask.reshape(-1, cols) if mask is not None else torch.ones_like(w2, dtype=torch.bool)
    d2 = torch.where(m2, torch.nan_to_num(g2 - w2, nan=float("inf")), torch.zeros_like(w2))
    rowrel = d2.norm(dim=1) / torch.where(m2, w2, torch.zeros_like(w2)).norm(dim=1).clamp_min(1e-30)
    rr = int(rowrel.argmax())
    n_bad = int((ratio > 1.0).sum())
    bad_rows = int((ratio.reshape(-1, cols) > 1.0).any(dim=1).sum())
    raise AssertionError(
        f"{name}: {n_bad} of {ratio.numel()} elements in {bad_rows} rows exceed their bound; worst err/bound {worst:.3g} at "
        f"{tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), want.shape))} = row {_mods(r)}, column {_mods(c)}: "
        f"got {float(g2[r, c]):.9g}, want {float(w2[r, c]):.9g}, bound {float(bound.reshape(-1, cols)[r, c]):.3g}; "
        f"worst row-relative error {float(rowrel[rr]):.3g} in row {_mods(rr)}")


# ------------------------------------------------------------------------------------------------ GEMM / implicit-GEMM conv
def gemm_reference(A, W, out, *, N, K, M=None, bias=None, epilogue=EPI_BIAS, gate=None, resid=None, conv=None, ps=None,
                   phase=None, abs_err=0.0, **_launch_only):
    """fp64 result and bound of one ``gemm`` launch (same keywords as HipOps.gemm), laid out like ``out``:
    -> (want, bound, mask); mask = the elements the launch writes (the index maps -- pixel shuffle, drop_first, phase scatter --
    are applied to the fp64 result exactly as tests/ops_reference.py applies them to the fp32 one).

        |err| <= u_out (|want| + b) + b,   b = 2 K u32 S,   S = |A| |W|^T + |bias|   [ |gate| S + |resid| with a gate / residual ]

    K = kt kh kw Cin for a conv.  gamma_K = K u32 is the textbook bound of a K-term fp32 dot product; the factor 2 covers an MFMA
    block, whose internal adds are not individually rounded to nearest.  Through SiLU / tanh-GELU the pre-activation bound is
    multiplied by the activation's Lipschitz constant and 8 u32 |want| is added for fast_exp2 / v_rcp; SwiGLU = silu(g) * i takes
    the product rule |i| L b_g + |silu(g)| b_i + L b_g b_i.
    ``abs_err``: an absolute term on the value before the store -- 2^-126 where a test drives results into fp32's denormal range,
    which the hardware may flush to zero (SwiGLU: times 1 + |i|, a flushed gate is multiplied by i)."""
    if phase is not None and getattr(phase, "quad", None) is not None:
        want = torch.full(out.shape, float("nan"), dtype=F64, device=out.device)
        bound = torch.zeros(out.shape, dtype=F64, device=out.device)
        mask = torch.zeros(out.shape, dtype=torch.bool, device=out.device)
        for qpy, qpx, qw, qb, qbb, _ in phase.quad:
            one = type(phase)(qpy, qpx, qbb, phase.t_stride)
            w1, b1, m1 = gemm_reference(A, qw, out, N=N, K=K, bias=qb, phase=one,
                                        conv=dataclasses.replace(conv, pad=(conv.pad[0], 1 - qpy, 1 - qpx)))
            want, bound, mask = torch.where(m1, w1, want), torch.where(m1, b1, bound), mask | m1
        return want, bound, mask
    conv_abs = None
    if conv is not None:
        conv_abs = dataclasses.replace(conv, halo=conv.halo.abs() if conv.halo is not None else None)
    acc = gemm_acc(A, W, N=N, K=K, M=M, conv=conv, dtype=F64)
    S = gemm_acc(A.abs(), W.abs(), N=N, K=K, M=M, conv=conv_abs, dtype=F64)
    M = acc.shape[0]
    k_red = conv.k[0] * conv.k[1] * conv.k[2] * conv.Cin if conv is not None else K
    c = 2.0 * k_red * U32
    if epilogue == EPI_SWIGLU:
        a4, s4 = acc.reshape(M, N // 32, 2, 16), S.reshape(M, N // 32, 2, 16)
        g, i, bg, bi = a4[:, :, 0], a4[:, :, 1], c * s4[:, :, 0], c * s4[:, :, 1]
        sg = F.silu(g)
        want = (sg * i).reshape(M, N // 2)
        b = (i.abs() * LIP_SILU * bg + sg.abs() * bi + LIP_SILU * bg * bi + abs_err * (1.0 + i.abs())).reshape(M, N // 2) + APPROX * want.abs()
    else:
        brow = gemm_bias_rows(bias, N, conv, phase, F64, acc.device)
        want = acc + brow
        b = c * (S + brow.abs())
        if epilogue == EPI_BIAS_GELU:
            want = F.gelu(want, approximate="tanh")
            b = LIP_GELU * b + APPROX * want.abs()
        elif epilogue == EPI_BIAS_SILU:
            want = F.silu(want)
            b = LIP_SILU * b + APPROX * want.abs()
        elif epilogue == EPI_RESID_GATE:
            if gate is not None:
                want = want * gate[:N].to(F64)
                b = b * gate[:N].to(F64).abs()
            if resid is not None:
                r = values(resid.reshape(M, -1)[:, :N])
                want = want + r
                b = b + c * r.abs()
        b = b + abs_err
    b = store_bound(want, b, out.dtype)
    full_w = torch.full(out.shape, float("nan"), dtype=F64, device=out.device)
    full_b = torch.zeros(out.shape, dtype=F64, device=out.device)
    mask = torch.zeros(out.shape, dtype=torch.bool, device=out.device)
    kw = dict(conv=conv, ps=ps, phase=phase)
    gemm_place(want, full_w, **kw)
    gemm_place(b, full_b, **kw)
    gemm_place(torch.ones_like(want, dtype=torch.bool), mask, **kw)
    return full_w, full_b, mask


def check_gemm(got, A, W, *, name="gemm", before=None, **kw):
    """``got``: the tensor a HipOps.gemm(A, W, got, **kw) launch wrote (pass the residual as it was BEFORE an in-place launch)."""
    want, bound, mask = gemm_reference(A, W, got, **kw)
    return check(name, got, want, bound, mask, before)


# ------------------------------------------------------------------------------------------------ window attention
def attn_reference(qkv, out, seq_rows, out_rows, cu, heads, head_dim, scale):
    """fp64 softmax(scale q k^T) v per window and head, and

        |err| <= u_out |want| + 2 2^-8 (P |V|) + 2 delta (P |V|),     delta = 2 D u32 scale max_row(|q| |k|^T)

    P = the fp64 softmax; delta = the error of a row's scores (a D-term bf16 MFMA dot product in fp32, factor 2 as in the GEMMs),
    which moves every probability by at most a factor exp(+-2 delta); the middle term = P rounded to bf16 before the PV product
    (numerator and denominator each move by 2^-8 relative).  -> (want, bound, mask) laid out like ``out``."""
    dev = qkv.device
    q3 = values(qkv).reshape(qkv.shape[0], 3, heads, head_dim)
    want = torch.full(out.shape, float("nan"), dtype=F64, device=dev)
    bound = torch.zeros(out.shape, dtype=F64, device=dev)
    mask = torch.zeros(out.shape, dtype=torch.bool, device=dev)
    cu_l = cu.tolist()
    for i in range(len(cu_l) - 1):
        src = seq_rows[cu_l[i]:cu_l[i + 1]].long()
        dst = out_rows[cu_l[i]:cu_l[i + 1]].long()
        for h0 in range(0, heads, 4):                                   # (four heads at a time: L x L fp64 temporaries)
            q, k, v = (q3[src, j, h0:h0 + 4].transpose(0, 1) for j in range(3))     # [h, L, D]
            P = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
            delta = 2.0 * head_dim * U32 * scale * (q.abs() @ k.abs().transpose(-1, -2)).amax(dim=-1, keepdim=True)   # [h, L, 1]
            w = P @ v
            pv = P @ v.abs()
            b = 2.0 * U_BF16 * pv + 2.0 * delta * pv
            cols = slice(h0 * head_dim, (h0 + q.shape[0]) * head_dim)
            want[dst, cols] = w.transpose(0, 1).reshape(len(src), -1)
            bound[dst, cols] = b.transpose(0, 1).reshape(len(src), -1)
        mask[dst] = True
    return want, store_bound(want, bound, out.dtype), mask


def check_attn(got, qkv, seq_rows, out_rows, cu, heads, head_dim, scale, *, name="attn_varlen", before=None):
    want, bound, mask = attn_reference(qkv, got, seq_rows, out_rows, cu, heads, head_dim, scale)
    return check(name, got, want, bound, mask, before)


# ------------------------------------------------------------------------------------------------ row-normalising kernels
def _row_bound(n, mag):
    """(n / 2 + 8) u32 mag: the fp32 sum of n squares (tree-shaped: far fewer than n sequential adds; n / 2 is what a plain loop
    over half the row would cost) enters through rsqrt with a factor 1/2; 8 u32 for v_rsq_f32 and the multiplies / fma behind it."""
    return (n / 2.0 + 8.0) * U32 * mag


def rmsnorm_mod_reference(x, eps, w=None, scale=None, shift=None, out_dtype=torch.bfloat16):
    """want = x rsqrt(mean(x^2) + eps) [w] [scale] + [shift]; bound u_out |want| + (dim / 2 + 8) u32 (|x inv w scale| + |shift|)."""
    xf = values(x)
    y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32)))
    for f in (w, scale):
        if f is not None:
            y = y * f.to(F64)
    mag = y.abs()
    if shift is not None:
        y = y + shift.to(F64)
        mag = mag + shift.to(F64).abs()
    return y, store_bound(y, _row_bound(x.shape[-1], mag), out_dtype)


def check_rmsnorm_mod(got, x, eps, w=None, scale=None, shift=None, *, name="rmsnorm_mod"):
    want, bound = rmsnorm_mod_reference(x, eps, w, scale, shift, got.dtype)
    return check(name, got, want, bound)


def qknorm_rope_reference(qkv, heads, pos, t_offset, cos_tab, sin_tab, wq, wk, eps):
    """q / k RMSNorm over 128 + interleaved-pair RoPE on the first 3 n_freq pairs, of the q and k columns of ``qkv`` AS IT WAS
    BEFORE the in-place launch.  Table rows are pos (+ t_offset on axis 0) CLAMPED to [0, n_pos - 1], as the kernel clamps them.
    -> (want, bound) [rows, 2 * heads * 128]; bound u_out |want| + (128 / 2 + 8) u32 (|t0 cos| + |t1 sin|), t = x inv w."""
    rows = qkv.shape[0]
    n_pos, nf = cos_tab.shape
    v = values(qkv).reshape(rows, 3, heads, 128)[:, :2]
    p = pos.long().clone()
    p[:, 0] += t_offset
    p = p.clamp(0, n_pos - 1)
    cos = torch.cat([cos_tab.to(F64)[p[:, a]] for a in range(3)], dim=-1)[:, None, None, :]        # [rows, 1, 1, 3 nf]
    sin = torch.cat([sin_tab.to(F64)[p[:, a]] for a in range(3)], dim=-1)[:, None, None, :]
    wgt = torch.stack([wq.to(F64), wk.to(F64)])[None, :, None, :]                                  # [1, 2, 1, 128]
    t = v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + float(torch.tensor(eps, dtype=torch.float32))) * wgt
    rot = t[..., :6 * nf].reshape(rows, 2, heads, 3 * nf, 2)
    x0, x1 = rot[..., 0], rot[..., 1]
    r = torch.stack((x0 * cos - x1 * sin, x1 * cos + x0 * sin), dim=-1).reshape(rows, 2, heads, 6 * nf)
    m = torch.stack(((x0 * cos).abs() + (x1 * sin).abs(), (x1 * cos).abs() + (x0 * sin).abs()), dim=-1).reshape(rows, 2, heads, 6 * nf)
    want = torch.cat([r, t[..., 6 * nf:]], dim=-1).reshape(rows, -1)
    mag = torch.cat([m, t[..., 6 * nf:].abs()], dim=-1).reshape(rows, -1)
    return want, store_bound(want, _row_bound(128, mag), qkv.dtype)


def check_qknorm_rope(got, qkv_before, heads, pos, t_offset, cos_tab, sin_tab, wq, wk, eps, *, name="qknorm_rope"):
    """q and k against their bounds, and the V columns bit-untouched."""
    want, bound = qknorm_rope_reference(qkv_before, heads, pos, t_offset, cos_tab, sin_tab, wq, wk, eps)
    n = 2 * heads * 128
    assert torch.equal(got[:, n:], qkv_before[:, n:]), f"{name}: V columns were written"
    return check(name, got[:, :n], want, bound)


def groupnorm_stats_reference(x, groups, slab_rows=None):
    """fp64 (sum, sum of squares) per (frame, group) and the bound of the kernel's fp32 stage: a thread adds n_t fp32 terms
    before the fp64 stages -- 4 per row (f0 + f1 + f2 + f3 into the running sum) over ceil(2048 / rstep) rows of its block,
    rstep = 256 / (C / 8) -- so |sum err| <= n_t u32 sum|x| and |sumsq err| <= n_t u32 sum x^2.  -> (want, bound) [T, groups, 2].
    ``slab_rows``: H rows at a time (fp64 temporaries of a large frame)."""
    T, H, W, C = x.shape
    rstep = 256 // (C // 8)
    n_t = 4 * -(-GN_ROWS_PER_BLOCK // rstep)
    want = torch.zeros(T, groups, 2, dtype=F64, device=x.device)
    mag = torch.zeros(T, groups, 2, dtype=F64, device=x.device)
    step = slab_rows or H
    for y0 in range(0, H, step):
        xg = values(x[:, y0:y0 + step]).reshape(T, -1, groups, C // groups)
        sq = xg.pow(2).sum(dim=(1, 3))
        want += torch.stack([xg.sum(dim=(1, 3)), sq], dim=-1)
        mag += torch.stack([xg.abs().sum(dim=(1, 3)), sq], dim=-1)
    return want, n_t * U32 * mag


def check_groupnorm_stats(got, x, groups, *, name="groupnorm_stats", slab_rows=None):
    want, bound = groupnorm_stats_reference(x, groups, slab_rows)
    return check(name, got, want, bound)


def _groupnorm_apply_from(x, mean, rstd, gamma, beta, silu, out_dtype):
    """want and bound of the apply pass for fp64 ``mean`` / ``rstd`` [T, groups] (groupnorm_apply_reference states the bound);
    also the normalised value (x - mean) rstd gamma before beta."""
    T, H, W, C = x.shape
    cpg = C // mean.shape[1]
    mean_c = mean.repeat_interleave(cpg, dim=1)[:, None, None, :]
    rstd_c = rstd.repeat_interleave(cpg, dim=1)[:, None, None, :]
    xf, g, b = values(x), gamma.to(F64), beta.to(F64)
    norm = (xf - mean_c) * rstd_c * g
    y = norm + b
    acc = _row_bound(1, (xf.abs() + mean_c.abs()) * rstd_c * g.abs() + b.abs())
    if silu:
        y = F.silu(y)
        acc = LIP_SILU * acc + APPROX * y.abs()
    return y, store_bound(y, acc, out_dtype), norm


def groupnorm_apply_reference(x, stats, gamma, beta, groups, eps, silu, out_dtype=torch.bfloat16, hw_total=None):
    """y = act((x - mean) rstd gamma + beta) from the GIVEN fp64 statistics (``hw_total``: rows of the whole frame when ``x`` is
    a slab of it).  The kernel evaluates x a + b with a = gamma rstd, b = beta - mean a in fp32, no reduction (n = 1):
    bound u_out |want| + (1 / 2 + 8) u32 mag with mag = (|x| + |mean|) rstd |gamma| + |beta| -- the terms that are actually
    rounded; through SiLU times its Lipschitz constant, + 8 u32 |want|."""
    T, H, W, C = x.shape
    cpg = C // groups
    n = float((hw_total if hw_total is not None else H * W) * cpg)
    mean = stats[..., 0].to(F64) / n
    var = (stats[..., 1].to(F64) / n - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    return _groupnorm_apply_from(x, mean, rstd, gamma, beta, silu, out_dtype)[:2]


def check_groupnorm_apply(got, x, stats, gamma, beta, groups, eps, silu, *, name="groupnorm_apply", slab_rows=None):
    """``slab_rows``: compare H rows at a time (fp64 temporaries of a whole 4K frame would not fit)."""
    T, H, W, C = x.shape
    step = slab_rows or H
    worst = 0.0
    for t in range(T if slab_rows else 1):
        ts = slice(t, t + 1) if slab_rows else slice(None)
        for y0 in range(0, H, step):
            want, bound = groupnorm_apply_reference(x[ts, y0:y0 + step], stats[ts], gamma, beta, groups, eps, silu, got.dtype, H * W)
            tag = name if not slab_rows else f"{name}[frame {t}, rows {y0}..]"
            worst = max(worst, check(tag, got.reshape(x.shape)[ts, y0:y0 + step], want, bound))
    return worst


GN_STATS_REL = 2.0 ** -10             # what the statistics may add to a normalised value: a quarter of one bf16 store roundoff


def two_pass_moments(x, groups):
    """fp64 mean and TWO-PASS variance per (frame, group) of the stored values: mean first (with one correction step: a device
    reduction may form it as sum * (1 / n), one ulp off), then mean((x - mean)^2) -- no cancellation, whatever mean / std is.
    -> (mean, var) [T, groups]."""
    T, H, W, C = x.shape
    xg = values(x).reshape(T, H * W, groups, C // groups)
    mean = xg.mean(dim=(1, 3))
    mean = mean + (xg - mean[:, None, :, None]).mean(dim=(1, 3))                   # (the fp64 mean's own rounding, taken out: a
    var = (xg - mean[:, None, :, None]).pow(2).mean(dim=(1, 3))                    # constant group has variance 0 EXACTLY)
    return mean, var


def groupnorm_reference(x, gamma, beta, groups, eps, silu, out_dtype=torch.bfloat16):
    """The COMPOSED GroupNorm (statistics pass + apply pass) against statistics the kernels had no part in: mean and two-pass
    variance in fp64 from the stored values.  Bound: groupnorm_apply_reference's, evaluated with these exact statistics, plus

        2^-10 |(x - mean) rstd gamma|        (times LIP_SILU under SiLU)

    for the statistics pass.  2^-10 is a REQUIREMENT, not a fit: the statistics may move a normalised value by a quarter of one
    bf16 store roundoff (2^-8), i.e. rstd by 2^-10 relative, i.e. var + eps by 2^-9 relative -- which check_groupnorm_variance
    states on the statistics themselves.  -> (want, bound)."""
    mean, var = two_pass_moments(x, groups)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(eps, dtype=torch.float32)))
    want, bound, norm = _groupnorm_apply_from(x, mean, rstd, gamma, beta, silu, out_dtype)
    return want, bound + (LIP_SILU if silu else 1.0) * GN_STATS_REL * norm.abs()


def check_groupnorm(got, x, gamma, beta, groups, eps, silu, *, name="groupnorm composed"):
    want, bound = groupnorm_reference(x, gamma, beta, groups, eps, silu, got.dtype)
    return check(name, got.reshape(x.shape), want, bound)


def check_groupnorm_variance(stats, x, groups, eps, *, name="groupnorm variance"):
    """The variance the apply pass derives from ``stats`` [T, groups, 2] (E[x^2] - mean^2 in fp64, clamped at 0, as
    groupnorm_apply_kernel forms it) against the two-pass variance of the stored values:

        |var_stats - var| <= 2^-9 (var + eps)        per (frame, group)

    -> worst |error| / bound.  A failure names the group, its rho = |mean| / std and both variances."""
    T, H, W, C = x.shape
    n = float(H * W * (C // groups))
    mean, var = two_pass_moments(x, groups)
    eps = float(torch.tensor(eps, dtype=torch.float32))
    m_s = stats[..., 0].to(F64) / n
    var_s = (stats[..., 1].to(F64) / n - m_s * m_s).clamp_min(0)
    bound = 2.0 * GN_STATS_REL * (var + eps)
    worst, ratio = worst_ratio(var_s, var, bound)
    _record(name, worst)
    if worst > 1.0:
        t, g = divmod(int(ratio.reshape(-1).argmax()), groups)
        rho = float(mean[t, g].abs() / var[t, g].sqrt().clamp_min(1e-300))
        raise AssertionError(
            f"{name}: {int((ratio > 1.0).sum())} of {ratio.numel()} (frame, group) variances exceed 2^-9 (var + eps); worst "
            f"err/bound {worst:.3g} in frame {t}, group {g} (rho = |mean| / std = {rho:.4g}, mean {float(mean[t, g]):.9g}): variance "
            f"from the statistics {float(var_s[t, g]):.9g}, two-pass variance {float(var[t, g]):.9g}")
    return worst


# ------------------------------------------------------------------------------------------------ softmax, small side kernels
def softmax_rows_reference(S, scale, out_dtype=torch.bfloat16):
    """P = softmax(scale S) over the last dimension; bound u_out want + 8 u32 (probabilities are <= 1: the exponent's and the
    sum's fp32 errors and fast_exp2 / the reciprocal are absolute errors of that size)."""
    want = torch.softmax(S.to(F64) * float(torch.tensor(scale, dtype=torch.float32)), dim=-1)
    return want, store_bound(want, torch.full_like(want, APPROX), out_dtype)


def check_softmax_rows(got, S, scale, *, name="softmax_rows"):
    want, bound = softmax_rows_reference(S, scale, got.dtype)
    return check(name, got, want, bound)


def rows_mean_reference(src, n_groups, rows_per_group, out_dtype=torch.bfloat16):
    """mean over the n_groups copies of each row: n = n_groups sequential fp32 adds, mag = mean |x|."""
    v = values(src).reshape(n_groups, rows_per_group, -1)
    want = v.mean(0)
    return want, store_bound(want, _row_bound(n_groups, v.abs().mean(0)), out_dtype)


def unpatchify_euler_reference(pred, x_t, out_shape, out_dtype=torch.bfloat16):
    """x_t - unpatchify(pred[:, :4C]) (or the prediction alone): an index map and one fp32 subtraction (u32 |want|)."""
    T, H, W, C = out_shape
    p = values(pred[:, :4 * C]).reshape(T, H // 2, W // 2, 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(T, H, W, C)
    want = values(x_t) - p if x_t is not None else p
    return want, store_bound(want, U32 * want.abs(), out_dtype)


# ------------------------------------------------------------------------------------------------ glue kernels of the engines
def ada_combine_reference(emb, params, slots):
    """out[v, i] = emb[6 i + slots[v]] + params[v, i] into fp32: ONE fp32 add of two bf16 values, and the fp32 store keeps the
    sum as it is -- bound u32 |want|.  -> (want, bound) [n_vec, dim]."""
    dim = params.shape[1]
    want = values(emb).reshape(dim, 6)[:, slots.long()].t() + values(params)
    return want, U32 * want.abs()


def check_ada_combine(got, emb, params, slots, *, name="ada_combine"):
    want, bound = ada_combine_reference(emb, params, slots)
    return check(name, got, want, bound)


def check_bits(name, got, want):
    """Pure data movement (patchify, im2col_causal): ``got`` must hold the BITS of ``want`` (the tests/ops_reference.py result,
    pad columns zero) -- a bound of zero on the bit patterns, so -0.0 is not 0.0 and a NaN payload is compared too.
    -> 0.0; a failure names the first differing element."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {tuple(got.shape)} {got.dtype} against {tuple(want.shape)} {want.dtype}"
    raw = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    diff = got.contiguous().view(raw) != want.contiguous().view(raw)
    n_bad = int(diff.sum())
    _record(name, float("inf") if n_bad else 0.0)
    if n_bad:
        flat = int(diff.reshape(-1).to(torch.uint8).argmax())
        cols = want.shape[-1]
        r, c = divmod(flat, cols)
        raise AssertionError(f"{name}: {n_bad} of {diff.numel()} elements do not hold the reference's bits; first at row {_mods(r)}, "
                             f"column {_mods(c)}: got {float(got.reshape(-1)[flat]):.9g}, want {float(want.reshape(-1)[flat]):.9g}")
    return 0.0


def patchify_reference(vid, out):
    """The 2 x 2 patch rows of ``vid`` [T, H, W, C] in the leading 4 C columns, zeros in the pad columns: the tests/ops_reference.py
    result in the storage dtype (compare with check_bits)."""
    from ops_reference import TorchOps
    return TorchOps(vid.device, vid.dtype).patchify(vid, torch.empty_like(out))


def im2col_causal_reference(x, out, conv):
    """The tap-major im2col rows of a causal conv (carried halo or replicated first frame in front, zero borders, zero pad
    columns): the tests/ops_reference.py result in the storage dtype (compare with check_bits)."""
    from ops_reference import TorchOps
    return TorchOps(x.device, x.dtype).im2col_causal(x, torch.empty_like(out), conv)


def blend_accumulate_reference(tile, acc_before, cnt_before, wy, wx, y0, x0):
    """acc[:, y0:y0+h, x0:x0+w] += tile (wy wx) in fp32, cnt[y0:y0+h, x0:x0+w] += wy wx (the kernel: by its t == 0 threads only --
    once per pixel, whatever T is).  Three fp32 roundings per element -- w = wy wx, tile w, the add -- so

        |acc err| <= 2 u32 |tile w| + u32 |want|        |cnt err| <= 2 u32 |w| + u32 |want|     (the second rounding is absent for cnt)

    mask = the tile's rectangle; everything outside keeps its bits.  -> ((want, bound, mask) of acc, (want, bound, mask) of cnt)."""
    T, h, w, C = tile.shape
    wgt = wy.to(F64)[:, None] * wx.to(F64)[None, :]
    res = []
    for before, add in ((acc_before, values(tile) * wgt[None, :, :, None]), (cnt_before, wgt)):
        want = torch.full(before.shape, float("nan"), dtype=F64, device=before.device)
        bound = torch.zeros(before.shape, dtype=F64, device=before.device)
        mask = torch.zeros(before.shape, dtype=torch.bool, device=before.device)
        rect = (Ellipsis, slice(y0, y0 + h), slice(x0, x0 + w)) if before.dim() == 2 else (slice(None), slice(y0, y0 + h), slice(x0, x0 + w))
        want[rect] = before.to(F64)[rect] + add
        bound[rect] = 2.0 * U32 * add.abs() + U32 * want[rect].abs()
        mask[rect] = True
        res.append((want, bound, mask))
    return res[0], res[1]


def check_blend_accumulate(acc, cnt, tile, acc_before, cnt_before, wy, wx, y0, x0, *, name="blend_accumulate"):
    (wa, ba, ma), (wc, bc, mc) = blend_accumulate_reference(tile, acc_before, cnt_before, wy, wx, y0, x0)
    return max(check(name + " acc", acc, wa, ba, ma, acc_before), check(name + " cnt", cnt.reshape(wc.shape), wc, bc, mc, cnt_before.reshape(wc.shape)))


def _f32(v):
    """a Python scalar as the C ABI receives it (a ``float`` argument)"""
    return float(torch.tensor(v, dtype=torch.float32))


def blend_finalize_reference(acc, cnt, c_take, scale=1.0, shift=0.0, out_dtype=torch.bfloat16):
    """want = (acc[..., :c_take] / max(cnt, 1e-6) - shift) scale.  q = acc / cnt may be formed with a reciprocal (APPROX |q|: v_rcp_f32
    and the multiply behind it); then the quotient, the subtraction and the product are rounded to fp32 -- three roundings, each
    at most u32 of the magnitudes that met, which (|q| + |shift|) |scale| covers in either order of evaluation (and under
    cancellation in q - shift):

        |err| <= u_out (|want| + b) + b,      b = (APPROX + 3 u32) (|q| + |shift|) |scale|

    -> (want, bound) [T, H, W, c_take]."""
    scale, shift = _f32(scale), _f32(shift)
    q = acc[..., :c_take].to(F64) / cnt.to(F64).clamp_min(_f32(1e-6)).reshape(1, acc.shape[1], acc.shape[2], 1)
    want = (q - shift) * scale
    return want, store_bound(want, (APPROX + 3.0 * U32) * (q.abs() + abs(shift)) * abs(scale), out_dtype)


def check_blend_finalize(got, acc, cnt, scale=1.0, shift=0.0, *, name="blend_finalize"):
    want, bound = blend_finalize_reference(acc, cnt, got.shape[-1], scale, shift, got.dtype)
    return check(name, got.reshape(want.shape), want, bound)


def affine_slice_reference(inp, c_out, scale=1.0, shift=0.0, out_dtype=torch.bfloat16):
    """want = (inp[..., :c_out] - shift) scale: two fp32 roundings (the subtraction, the product), then the store:

        |err| <= u_out (|want| + b) + b,      b = 2 u32 (|x| + |shift|) |scale|

    -> (want, bound) [..., c_out]."""
    scale, shift = _f32(scale), _f32(shift)
    x = values(inp[..., :c_out])
    want = (x - shift) * scale
    return want, store_bound(want, 2.0 * U32 * (x.abs() + abs(shift)) * abs(scale), out_dtype)


def check_affine_slice(got, inp, scale=1.0, shift=0.0, *, name="affine_slice"):
    want, bound = affine_slice_reference(inp, got.shape[-1], scale, shift, got.dtype)
    return check(name, got.reshape(want.shape), want, bound)

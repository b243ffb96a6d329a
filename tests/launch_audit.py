"""TEST INFRASTRUCTURE: every launch an ENGINE issues, held to the per-element bounds of tests/local_error.py.

The kernel tests choose their cases by hand; the engine tests compare a whole forward pass norm-wise (2e-2 for the VAE, 8e-3 for the
DiT: a random-weight network amplifies bf16 noise that far).  Between the two, the launches the engines actually issue -- M = 1
GEMMs, row-offset views, in-place residuals, frames below one patch, one-frame slices behind a carried halo, the causal-head pair,
quad phase launches sharing one partial buffer -- were never checked element by element.  ``audited(ops_cls)`` closes that:

    ops = audited(HipOps)("cuda:0")            # or audited(TorchOps)("cpu", act_dtype=torch.bfloat16): same method surface
    VideoVAEEngine(cfg, sd, ops).decode(z)     # the engine runs as always; nothing raises inside it
    ops.assert_clean()                         # raises ONCE, listing every offending launch

Per call of a data-path op the subclass clones what the launch may overwrite and the reference needs (an aliased residual, qkv of the
in-place q/k norm, acc / cnt of the tile blend) and the output's prior bits, lets the base class launch, then computes the fp64
reference and bound on the tensor's own device and records: sequence number, op, kernel class (HipOps: svr_gemm_kernel_class; else
None), shapes, storage kinds, the flags that tell the engines' forms apart, the worst err / bound, and whether an element outside the
launch's mask changed bits.  No allowed share of outliers: one element over its bound fails the launch.  Fused GroupNorm statistics
are compared with an fp64 reduction of the STORED output (measure and thresholds of tests/test_gpu_conv_mfma16.py: rel_err of the sums
< 1e-5, of the sums of squares < 1e-6); for launches sharing a ``gn_shared`` dict the output tensor is remembered per dict and the
check happens in gn_shared_stats.  A statistic that is None (the kernel does not fuse) is recorded, not failed.
Nested calls (HipOps.gemm issuing four phase launches when the library declines a quad, TorchOps.gemm calling itself): the
outermost call is the audited one.

``FusingTorchOps``: the CPU double with the fused statistics HipOps delivers (an fp64 reduction of what it stored), so that the
statistics path of the audit -- and a fault in it -- can be exercised without a GPU.
``vae_forms`` / ``dit_forms``: the engines' forms as predicates over the records; a test asserts them so that an audit cannot pass by
auditing nothing, and so that an engine change that stops issuing a form is noticed."""
import dataclasses
from typing import Optional

import torch

import local_error as le
from ops_reference import TorchOps, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_SILU, EPI_RESID_GATE, EPI_SWIGLU, H16

F64 = torch.float64
STATS_SUM_REL, STATS_SQ_REL = 1e-5, 1e-6           # tests/test_gpu_conv_mfma16.py
FUSING_CLASSES = ("conv_halo", "conv_thin_in", "conv_subpixel")      # the kernels with GroupNorm statistics in their epilogue
_KIND = {torch.bfloat16: "bf16", torch.float32: "fp32", H16: "h16", F64: "fp64"}


def kind(t):
    return None if t is None else _KIND.get(t.dtype, str(t.dtype))


@dataclasses.dataclass
class Record:
    seq: int
    op: str
    kernel_class: Optional[str] = None
    shapes: dict = dataclasses.field(default_factory=dict)
    kinds: dict = dataclasses.field(default_factory=dict)
    flags: dict = dataclasses.field(default_factory=dict)
    worst: float = 0.0                 # worst err / bound over the launch's elements
    stray: bool = False                # an element outside the launch's mask changed bits
    failures: list = dataclasses.field(default_factory=list)

    def describe(self):
        f = ", ".join(f"{k}={v}" for k, v in self.flags.items() if v not in (None, False, 0, ()))
        s = ", ".join(f"{k}{list(v)}" for k, v in self.shapes.items())
        k = ", ".join(f"{k}:{v}" for k, v in self.kinds.items() if v)
        return f"launch #{self.seq} {self.op} [{self.kernel_class}] {s} ({k}) {f}"


def _rel(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _same_start(a, b):
    return a is not None and b is not None and a.data_ptr() == b.data_ptr() and a.dtype == b.dtype


def _overlaps(a, b):
    if a is None or b is None or a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return False
    return True


class _Audit:
    """The overriding half of an audited ops class (see the module docstring); the other base is HipOps or TorchOps."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.records = []
        self._depth = 0
        self._shared = {}                       # id(gn_shared dict) -> {"dict", "out" (the whole tensor), "records"}
        if hasattr(self, "record_kernel_class"):
            self.record_kernel_class = True

    # ------------------------------------------------------------------ bookkeeping
    def _begin(self, op, **flags):
        rec = Record(len(self.records), op, flags=flags)
        self.records.append(rec)
        return rec

    def _judge(self, rec, got, want, bound, mask=None, before=None, what=""):
        """local_error.check semantics, recorded instead of raised."""
        name = f"#{rec.seq} {rec.op}{what}"
        worst, _ = le.worst_ratio(got, want, bound, mask)
        rec.worst = max(rec.worst, worst)
        if worst > 1.0:
            try:
                le.check(name, got, want, bound, mask)
            except AssertionError as e:
                rec.failures.append(str(e))
        if mask is not None and before is not None:
            raw = torch.int16 if got.element_size() == 2 else torch.int32
            stray = (got.view(raw) != before.view(raw)) & ~mask
            if bool(stray.any()):
                rec.stray = True
                rec.failures.append(f"{name}: the launch wrote {int(stray.sum())} elements that are not its own")

    def _judge_bits(self, rec, got, want):
        raw = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
        if got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.contiguous().view(raw), want.contiguous().view(raw)):
            return
        try:
            le.check_bits(f"#{rec.seq} {rec.op}", got, want)
        except AssertionError as e:
            rec.worst = float("inf")
            rec.failures.append(str(e))

    def _judge_stats(self, rec, stats, stored, groups):
        """fused statistics [frames, groups, 2] against the fp64 reduction of the stored tensor [frames, H, W, C]"""
        T, C = stored.shape[0], stored.shape[-1]
        xg = le.values(stored).reshape(T, -1, groups, C // groups)
        want = torch.stack([xg.sum(dim=(1, 3)), xg.pow(2).sum(dim=(1, 3))], dim=-1)
        e_sum, e_sq = _rel(stats[..., 0], want[..., 0]), _rel(stats[..., 1], want[..., 1])
        rec.flags["stats_rel"] = (e_sum, e_sq)
        if not (e_sum < STATS_SUM_REL and e_sq < STATS_SQ_REL):        # (a NaN fails)
            per_frame = ((stats.to(F64) - want).abs().amax(dim=(1, 2)) / want.abs().amax(dim=(1, 2)).clamp_min(1e-300)).tolist()
            rec.failures.append(f"#{rec.seq} {rec.op}: fused GroupNorm statistics are not those of the stored output: rel_err of the sums "
                                f"{e_sum:.3g} (< {STATS_SUM_REL:g}), of the sums of squares {e_sq:.3g} (< {STATS_SQ_REL:g}); worst relative "
                                f"deviation per frame " + " ".join(f"{v:.2g}" for v in per_frame))

    def failed(self):
        return [r for r in self.records if r.failures]

    def assert_clean(self):
        bad = self.failed()
        if bad:
            lines = [f"{len(bad)} of {len(self.records)} audited launches are outside their bounds:"]
            for r in bad:
                lines.append("  " + r.describe())
                lines.extend("      " + m for m in r.failures)
            raise AssertionError("\n".join(lines))
        return len(self.records)

    def headroom(self):
        """{(op, kernel class): worst err / bound}"""
        out = {}
        for r in self.records:
            key = (r.op, r.kernel_class)
            out[key] = max(out.get(key, 0.0), r.worst)
        return out

    def log_headroom(self, scenario):
        """One line per (scenario, op, kernel class) through local_error's record (printed; appended to SVR_LOCAL_ERROR_LOG)."""
        for (op, cls), worst in sorted(self.headroom().items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
            le._record(f"{scenario} | {op} | {cls}", worst)

    # ------------------------------------------------------------------ GEMM / conv
    def gemm(self, A, W, out, **kw):
        if self._depth:
            return super().gemm(A, W, out, **kw)
        conv, ps, phase, resid = kw.get("conv"), kw.get("ps"), kw.get("phase"), kw.get("resid")
        gn_groups, gn_shared, epi = kw.get("gn_groups", 0), kw.get("gn_shared"), kw.get("epilogue", EPI_BIAS)
        rec = self._begin(
            "gemm", epilogue={EPI_BIAS: "bias", EPI_BIAS_SILU: "silu", EPI_RESID_GATE: "resid_gate", EPI_SWIGLU: "swiglu",
                              EPI_BIAS_GELU: "gelu"}[epi],
            M=(conv.To * conv.Ho * conv.Wo) if conv is not None else (kw.get("M") or A.numel() // A.shape[-1]), N=kw["N"], K=kw["K"],
            conv=conv is not None, taps=tuple(conv.k) if conv is not None else (), stride=tuple(conv.stride) if conv is not None else (),
            in_frames=conv.T if conv is not None else 0, pad_t=conv.pad[0] if conv is not None else 0,
            halo_frames=conv.halo.shape[0] if conv is not None and conv.halo is not None else 0,
            carried_halo=conv is not None and conv.halo is not None,
            frame_voxels=conv.H * conv.W if conv is not None else 0,
            phase=phase is not None, quad=phase is not None and getattr(phase, "quad", None) is not None, ps=ps is not None,
            stats_asked=gn_groups > 0, stats_delivered=False, shared=gn_shared is not None,
            resid=resid is not None, resid_is_out=_same_start(resid, out), gate=kw.get("gate") is not None,
            w_frag=kw.get("W_frag") is not None)
        rec.shapes = dict(A=A.shape, W=W.shape, out=out.shape)
        rec.kinds = dict(A=kind(A), out=kind(out), resid=kind(resid))
        before = out.clone()
        resid_ref = resid.clone() if _overlaps(resid, out) else resid
        self._depth += 1
        try:
            res = super().gemm(A, W, out, **kw)
        finally:
            self._depth -= 1
        rec.kernel_class = getattr(self, "last_kernel_class", None)
        ref_kw = {k: v for k, v in kw.items() if k in ("N", "K", "M", "bias", "epilogue", "gate", "conv", "ps", "phase")}
        want, bound, mask = le.gemm_reference(A, W, out, resid=resid_ref, **ref_kw)
        self._judge(rec, out, want, bound, mask, before)
        if gn_groups > 0 and gn_shared is None:
            stats = res[1]
            rec.flags["stats_delivered"] = stats is not None
            if stats is not None:
                self._judge_stats(rec, stats, out.reshape(conv.To, conv.Ho, conv.Wo, -1), gn_groups)
        elif gn_groups > 0:
            ent = self._shared.setdefault(id(gn_shared), dict(dict=gn_shared, records=[], groups=gn_groups))
            f0, frames = int(gn_shared["frame0"]), int(gn_shared["frames"])
            ent["out"] = torch.as_strided(out, (frames,) + tuple(out.shape[1:]), out.stride(), out.storage_offset() - f0 * out.stride(0))
            ent["records"].append(rec)
        return res

    def _gn_shared_stats(self, gn_shared):
        rec = self._begin("gn_shared_stats", stats_asked=True, stats_delivered=False)
        stats = super().gn_shared_stats(gn_shared)
        ent = self._shared.pop(id(gn_shared), None)
        rec.flags["stats_delivered"] = stats is not None
        rec.flags["launches"] = tuple(r.seq for r in ent["records"]) if ent else ()
        if stats is not None:
            if ent is None:
                rec.failures.append(f"#{rec.seq} gn_shared_stats: statistics delivered for a dict no audited launch shared")
            else:
                rec.shapes = dict(out=ent["out"].shape, stats=stats.shape)
                rec.kinds = dict(out=kind(ent["out"]))
                rec.kernel_class = ent["records"][-1].kernel_class
                for r in ent["records"]:
                    r.flags["stats_delivered"] = True
                self._judge_stats(rec, stats, ent["out"], ent["groups"])
        return stats

    # ------------------------------------------------------------------ DiT side kernels
    def rmsnorm_mod(self, x, out, eps, w=None, scale=None, shift=None):
        rec = self._begin("rmsnorm_mod", w=w is not None, scale=scale is not None, shift=shift is not None)
        rec.shapes, rec.kinds = dict(x=x.shape), dict(x=kind(x), out=kind(out))
        res = super().rmsnorm_mod(x, out, eps, w=w, scale=scale, shift=shift)
        want, bound = le.rmsnorm_mod_reference(x, eps, w, scale, shift, out.dtype)
        self._judge(rec, out, want, bound)
        return res

    def ada_combine(self, emb, params, slots, out):
        rec = self._begin("ada_combine")
        rec.shapes, rec.kinds = dict(params=params.shape), dict(out=kind(out))
        res = super().ada_combine(emb, params, slots, out)
        self._judge(rec, out, *le.ada_combine_reference(emb, params, slots))
        return res

    def qknorm_rope(self, qkv, heads, pos, t_offset, cos_tab, sin_tab, wq, wk, eps):
        rec = self._begin("qknorm_rope", heads=heads, t_offset=t_offset)
        rec.shapes, rec.kinds = dict(qkv=qkv.shape, tab=cos_tab.shape), dict(qkv=kind(qkv))
        before = qkv.clone()
        res = super().qknorm_rope(qkv, heads, pos, t_offset, cos_tab, sin_tab, wq, wk, eps)
        w2, b2 = le.qknorm_rope_reference(before, heads, pos, t_offset, cos_tab, sin_tab, wq, wk, eps)
        n = w2.shape[1]
        want = torch.full(qkv.shape, float("nan"), dtype=F64, device=qkv.device)
        bound = torch.zeros(qkv.shape, dtype=F64, device=qkv.device)
        mask = torch.zeros(qkv.shape, dtype=torch.bool, device=qkv.device)
        want[:, :n], bound[:, :n], mask[:, :n] = w2, b2, True          # (the V columns keep their bits)
        self._judge(rec, qkv, want, bound, mask, before)
        return res

    def attn_varlen(self, qkv, out, seq_rows, out_rows, cu, max_len, heads, head_dim, scale):
        rec = self._begin("attn_varlen", heads=heads, head_dim=head_dim, windows=cu.numel() - 1, max_len=max_len,
                          out_rows_differ=not torch.equal(seq_rows, out_rows))
        rec.shapes, rec.kinds = dict(qkv=qkv.shape, out=out.shape), dict(qkv=kind(qkv), out=kind(out))
        before = out.clone()
        res = super().attn_varlen(qkv, out, seq_rows, out_rows, cu, max_len, heads, head_dim, scale)
        want, bound, mask = le.attn_reference(qkv, out, seq_rows, out_rows, cu, heads, head_dim, scale)
        self._judge(rec, out, want, bound, mask, before)
        return res

    def softmax_rows(self, S, P, scale):
        rec = self._begin("softmax_rows")
        rec.shapes, rec.kinds = dict(S=S.shape), dict(S=kind(S), P=kind(P))
        res = super().softmax_rows(S, P, scale)
        self._judge(rec, P, *le.softmax_rows_reference(S, scale, P.dtype))
        return res

    def rows_mean(self, src, dst, n_groups, rows_per_group):
        rec = self._begin("rows_mean", n_groups=n_groups, rows_per_group=rows_per_group)
        rec.shapes, rec.kinds = dict(src=src.shape, dst=dst.shape), dict(src=kind(src), dst=kind(dst))
        res = super().rows_mean(src, dst, n_groups, rows_per_group)
        self._judge(rec, dst, *le.rows_mean_reference(src, n_groups, rows_per_group, dst.dtype))
        return res

    def patchify(self, vid, out):
        rec = self._begin("patchify")
        rec.shapes, rec.kinds = dict(vid=vid.shape, out=out.shape), dict(out=kind(out))
        res = super().patchify(vid, out)
        self._judge_bits(rec, out, le.patchify_reference(vid, out))
        return res

    def unpatchify_euler(self, pred, x_t, out):
        rec = self._begin("unpatchify_euler", euler=x_t is not None)
        rec.shapes, rec.kinds = dict(pred=pred.shape, out=out.shape), dict(out=kind(out))
        res = super().unpatchify_euler(pred, x_t, out)
        self._judge(rec, out, *le.unpatchify_euler_reference(pred, x_t, out.shape, out.dtype))
        return res

    # ------------------------------------------------------------------ VAE side kernels
    def groupnorm_stats(self, x, stats, groups):
        rec = self._begin("groupnorm_stats", groups=groups)
        rec.shapes, rec.kinds = dict(x=x.shape), dict(x=kind(x))
        res = super().groupnorm_stats(x, stats, groups)
        self._judge(rec, stats, *le.groupnorm_stats_reference(x, groups))
        return res

    def groupnorm_apply(self, x, out, stats, gamma, beta, groups, eps, silu):
        rec = self._begin("groupnorm_apply", groups=groups, silu=bool(silu))
        rec.shapes, rec.kinds = dict(x=x.shape), dict(x=kind(x), out=kind(out))
        res = super().groupnorm_apply(x, out, stats, gamma, beta, groups, eps, silu)
        want, bound = le.groupnorm_apply_reference(x, stats, gamma, beta, groups, eps, silu, out.dtype)
        self._judge(rec, out.reshape(x.shape), want, bound)
        return res

    def im2col_causal(self, x, out, conv):
        rec = self._begin("im2col_causal", taps=tuple(conv.k), stride=tuple(conv.stride), in_frames=conv.T,
                          carried_halo=conv.halo is not None)
        rec.shapes, rec.kinds = dict(x=x.shape, out=out.shape), dict(out=kind(out))
        res = super().im2col_causal(x, out, conv)
        self._judge_bits(rec, out, le.im2col_causal_reference(x, out, conv))
        return res

    def blend_accumulate(self, tile, acc, cnt, wy, wx, y0, x0):
        rec = self._begin("blend_accumulate", y0=y0, x0=x0)
        rec.shapes, rec.kinds = dict(tile=tile.shape, acc=acc.shape), dict(tile=kind(tile), acc=kind(acc))
        acc0, cnt0 = acc.clone(), cnt.clone()
        res = super().blend_accumulate(tile, acc, cnt, wy, wx, y0, x0)
        (wa, ba, ma), (wc, bc, mc) = le.blend_accumulate_reference(tile, acc0, cnt0.reshape(acc.shape[1], acc.shape[2]), wy, wx, y0, x0)
        self._judge(rec, acc, wa, ba, ma, acc0, " acc")
        self._judge(rec, cnt.reshape(wc.shape), wc, bc, mc, cnt0.reshape(wc.shape), " cnt")
        return res

    def blend_finalize(self, acc, cnt, out, scale=1.0, shift=0.0):
        rec = self._begin("blend_finalize", scale=scale, shift=shift)
        rec.shapes, rec.kinds = dict(acc=acc.shape, out=out.shape), dict(out=kind(out))
        res = super().blend_finalize(acc, cnt, out, scale, shift)
        want, bound = le.blend_finalize_reference(acc, cnt, out.shape[-1], scale, shift, out.dtype)
        self._judge(rec, out.reshape(want.shape), want, bound)
        return res

    def affine_slice(self, inp, out, scale=1.0, shift=0.0):
        rec = self._begin("affine_slice", scale=scale, shift=shift)
        rec.shapes, rec.kinds = dict(inp=inp.shape, out=out.shape), dict(out=kind(out))
        res = super().affine_slice(inp, out, scale, shift)
        want, bound = le.affine_slice_reference(inp, out.shape[-1], scale, shift, out.dtype)
        self._judge(rec, out.reshape(want.shape), want, bound)
        return res


_classes = {}


def audited(ops_cls):
    """-> a subclass of ``ops_cls`` (HipOps, TorchOps or a subclass of either), constructed like it, that audits every data-path
    launch into ``.records`` (see the module docstring).  gn_shared_stats is overridden only where the base has it: its presence
    is how the VAE engine learns that the ops fuse statistics across phase launches."""
    if ops_cls not in _classes:
        ns = {"gn_shared_stats": _Audit._gn_shared_stats} if hasattr(ops_cls, "gn_shared_stats") else {}
        _classes[ops_cls] = type("Audited" + ops_cls.__name__, (_Audit, ops_cls), ns)
    return _classes[ops_cls]


# ------------------------------------------------------------------------------------------------ the CPU double that fuses statistics
class FusingTorchOps(TorchOps):
    """TorchOps delivering the fused GroupNorm statistics of a conv launch the way HipOps does -- ``(out, stats)`` with the fp64
    (sum, sum of squares) per (frame, group) of the STORED output, and the ``gn_shared`` protocol of the phase launches."""

    @staticmethod
    def _sums(stored, groups):
        T, C = stored.shape[0], stored.shape[-1]
        xg = le.values(stored).reshape(T, -1, groups, C // groups)
        return torch.stack([xg.sum(dim=(1, 3)), xg.pow(2).sum(dim=(1, 3))], dim=-1)

    def pack_conv_frag(self, W, kt, Cin, N, taps=(3, 3)):
        """Stands for the fragment-ordered copy (same geometries as HipOps.pack_conv_frag; this double never reads it): with it the VAE
        engine issues its quad phase launches."""
        kh, kw = taps
        if Cin % 64 or N % 128 or W.shape[1] != kt * kh * kw * Cin or (kh, kw) not in ((3, 3), (2, 2)):
            return None
        return W[:N].reshape(-1).clone()

    def gemm(self, A, W, out, *, gn_groups=0, gn_shared=None, **kw):
        conv, phase = kw.get("conv"), kw.get("phase")
        super().gemm(A, W, out, **kw)
        if not gn_groups:
            return out
        if conv is None:
            return out, None
        if gn_shared is None:
            return out, self._sums(out.reshape(conv.To, conv.Ho, conv.Wo, -1), gn_groups)
        if "partial" not in gn_shared:
            gn_shared.update(ok=True, groups=gn_groups, partial=torch.zeros(gn_shared["frames"], gn_groups, 2, dtype=F64, device=out.device))
        o4 = out.reshape(-1, 2 * conv.Ho, 2 * conv.Wo, kw["N"])[0:(conv.To - 1) * phase.t_stride + 1:phase.t_stride]
        if phase.quad is None:
            o4 = o4[:, phase.py::2, phase.px::2]
        f0 = int(gn_shared["frame0"])
        gn_shared["partial"][f0:f0 + (conv.To - 1) * phase.t_stride + 1:phase.t_stride] += self._sums(o4, gn_groups)
        return out

    def gn_shared_stats(self, gn_shared):
        return gn_shared["partial"].clone() if gn_shared.get("ok", False) and "partial" in gn_shared else None


# ------------------------------------------------------------------------------------------------ the engines' forms
def _gemms(records):
    return [r for r in records if r.op == "gemm"]


def vae_forms(records):
    """{form: does any record show it} for the forms the VAE engine is known to issue (kernel classes are a GPU matter: the
    caller checks them)."""
    g = _gemms(records)
    convs = [r for r in g if r.flags["conv"]]
    ops_seen = {r.op for r in records}
    return {
        "conv with a carried halo": any(r.flags["carried_halo"] for r in convs),
        "carried halo of fewer frames than kt - 1": any(r.flags["carried_halo"] and not r.flags["phase"] and r.flags["halo_frames"] < r.flags["taps"][0] - 1 for r in convs),
        "conv with a single input frame": any(r.flags["in_frames"] == 1 for r in convs),
        "one-frame slice behind a carried two-frame halo": any(r.flags["in_frames"] == 1 and r.flags["halo_frames"] == 2 for r in convs),
        "frame smaller than one 16x32 patch": any(0 < r.flags["frame_voxels"] < 16 * 32 and r.flags["taps"][1:] == (3, 3) for r in convs),
        "two-tap causal-head pair": any(a.flags["taps"][:1] == (2,) and a.flags["in_frames"] == 1 and not a.flags["phase"] and b.flags["conv"] and b.flags["taps"][:1] == (3,) and b.flags["pad_t"] == 1
                                        for a, b in zip(g, g[1:]) if a.flags["conv"]),
        "quad phase launch": any(r.flags["quad"] for r in convs),
        "phase launches sharing one statistics buffer": any(r.flags["shared"] for r in convs),
        "strided conv": any(r.flags["stride"][1:] == (2, 2) for r in convs),
        "strided conv with a carried halo": any(r.flags["stride"] == (2, 2, 2) and r.flags["carried_halo"] for r in convs),
        "strided conv without a carried halo": any(r.flags["stride"][1:] == (2, 2) and not r.flags["carried_halo"] for r in convs),
        "conv_in as im2col + GEMM": "im2col_causal" in ops_seen,
        "1x1x1 shortcut as a GEMM with a wide residual trunk": any(not r.flags["conv"] and r.flags["epilogue"] == "bias" and r.kinds["out"] in ("h16", "fp32") for r in g),
        "GEMM with a wide residual read from elsewhere": any(not r.flags["conv"] and r.flags["resid"] and not r.flags["resid_is_out"] and r.kinds["resid"] in ("h16", "fp32") for r in g),
        "conv with a wide residual": any(r.flags["resid"] and r.kinds["resid"] in ("h16", "fp32") for r in convs),
        "fused mid-block attention (one head as wide as the block)": any(r.op == "attn_varlen" and r.flags["heads"] == 1 for r in records),
        "mid-block attention as GEMM, softmax_rows, GEMM": "softmax_rows" in ops_seen,
        "tile blending": {"blend_accumulate", "blend_finalize", "affine_slice"} <= ops_seen,
        "groupnorm_stats and groupnorm_apply": {"groupnorm_stats", "groupnorm_apply"} <= ops_seen,
    }


def dit_forms(records):
    g = _gemms(records)
    return {
        "M = 1 GEMM with SiLU": any(r.flags["M"] == 1 and r.flags["epilogue"] == "silu" for r in g),
        "GEMM on a row-offset view of the text rows": any(r.flags["M"] == 58 and r.shapes["out"][0] == 58 for r in g),
        "GEMM with resid is out and h16 output": any(r.flags["resid_is_out"] and r.kinds["out"] == "h16" for r in g),
        "SwiGLU GEMM": any(r.flags["epilogue"] == "swiglu" for r in g),
        "tanh-GELU GEMM": any(r.flags["epilogue"] == "gelu" for r in g),
        "attn_varlen with out_rows != seq_rows": any(r.op == "attn_varlen" and r.flags["out_rows_differ"] for r in records),
        "rows_mean": any(r.op == "rows_mean" for r in records),
        "Euler un-patchify": any(r.op == "unpatchify_euler" and r.flags["euler"] for r in records),
    }

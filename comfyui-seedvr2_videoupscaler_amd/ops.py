"""Torch-tensor front end of the C ABI: validates layouts, passes raw device pointers and the current
HIP stream.  PyTorch is used for device memory and streams only; all arithmetic happens in
libseedvr2_hip.so.  Every method raises if the library is missing or a tensor is not on the GPU.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from . import hip_lib
from .hip_lib import EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_SILU, EPI_RESID_GATE, EPI_SWIGLU  # noqa: F401 (re-export)

BF16 = torch.bfloat16
# "h16": the 2-byte WIDE storage format of tensors that are not MFMA operands (SVR_STORE_H16 in include/seedvr2_hip.h): a
# torch.float16 tensor whose elements hold x * 2^-6.  Only the library's kernels interpret it (GroupNorm, residual adds);
# h16_to_float() is for tests and debugging.
H16 = torch.float16
H16_SCALE = 2.0 ** -6
STORE_BF16, STORE_FP32, STORE_H16 = 0, 1, 2
_KIND = {BF16: STORE_BF16, torch.float32: STORE_FP32, H16: STORE_H16}


def store_kind(t: torch.Tensor) -> int:
    try:
        return _KIND[t.dtype]
    except KeyError:
        raise ValueError(f"activation storage must be bf16, fp32 or h16 (torch.float16), got {t.dtype}") from None


def h16_to_float(t: torch.Tensor) -> torch.Tensor:
    return t.float() * (1.0 / H16_SCALE) if t.dtype == H16 else t.float()


def on_device(t: torch.Tensor, device: torch.device) -> bool:
    return t.device == device or (t.device.type == "cuda" == device.type and t.device.index == (device.index or 0))


def clip_args(name, frames, device, *, channels="frames must have C = 3 or 4", min_hw=None, before=None, after=None):
    """What the entry points that read a clip check first -> (T, H, W, C, kind): frames [T, H, W, C] in fp32 or bf16, C = 3 or 4
    said in the caller's words (``channels``; None: the caller's ``before`` judges C), every size positive (``min_hw``: H and W at
    least that, spelled out; None: "at least one pixel"), dense and on ``device``.  ``before`` / ``after``: the caller's own
    checks of (T, H, W, C), run just before / just after the sizes; each returns its complaint or None."""
    if frames.dim() != 4 or frames.dtype not in (torch.float32, BF16):
        raise ValueError(f"{name}: frames must be [T, H, W, C] in fp32 or bf16, got {tuple(frames.shape)} {frames.dtype}")
    T, H, W, Cn = frames.shape
    if channels and Cn not in (3, 4):
        raise ValueError(f"{name}: {channels}, got C = {Cn}")

    def own(check):
        why = check(T, H, W, Cn) if check else None
        if why:
            raise ValueError(f"{name}: {why}")

    own(before)
    if T < 1 or min(H, W) < (min_hw or 1):
        sizes = "at least one pixel" if min_hw is None else f"T >= 1 frames of H >= {min_hw}, W >= {min_hw}"
        raise ValueError(f"{name}: frames must hold {sizes}, got {tuple(frames.shape)}")
    own(after)
    if not on_device(frames, device):
        raise ValueError(f"{name}: frames must live on {device}, got {frames.device}")
    if not frames.is_contiguous():
        raise ValueError(f"{name}: frames must be contiguous")
    return T, H, W, Cn, store_kind(frames)                  # (fp32 or bf16 by now: SVR_STORE_FP32 / SVR_STORE_BF16)


@dataclass
class Conv3dGeom:
    """Causal conv geometry over an NDHWC input (see svr_conv_geom in include/seedvr2_hip.h)."""
    T: int
    H: int
    W: int
    Cin: int
    To: int
    Ho: int
    Wo: int
    k: tuple          # (kt, kh, kw)
    stride: tuple     # (st, sh, sw)
    pad: tuple        # (pt, ph, pw) front pads
    halo: Optional[torch.Tensor] = None   # [halo_frames, H, W, Cin] bf16


@dataclass
class PixelShuffleGeom:
    F: int
    H: int
    W: int
    rz: int
    C: int
    drop_first: bool


@dataclass
class PhaseScatter:
    """Sub-pixel convolution launch: the conv's output voxel (t, y, x) lands at out[t * t_stride, 2y + py, 2x + px] (``out``
    = the upsampled tensor from the launch's first frame on); ``bias_border`` fp32 [3, N]: bias on the voxels whose window
    loses its border tap (row border | column border | both)."""
    py: int
    px: int
    bias_border: Optional[torch.Tensor] = None
    t_stride: int = 1
    # quad launch (ABI v6): ALL four spatial phases in one launch -- a list of four (py, px, W, bias, bias_border, W_frag) in
    # any order; py / px / bias_border above and the call's own W / bias / W_frag / conv pads then describe phase (0, 0) only
    # as a fallback (HipOps.gemm issues the four launches itself when the library does not take the quad form)
    quad: Optional[list] = None


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def fill_gemm_args(A, W, out, *, N, K, M=None, bias=None, epilogue=EPI_BIAS, gate=None, resid=None, out_f32=False,
                   conv: Optional[Conv3dGeom] = None, ps: Optional[PixelShuffleGeom] = None, lda=None, ldc=None, ldr=None,
                   W_frag=None, phase: Optional[PhaseScatter] = None, zeros_ptr: int = 0, chk=None, ptr=None):
    """svr_gemm_args for one ``gemm`` call (layout checks included).  ``chk(tensor, dtype, name)`` validates device / dtype /
    contiguity (HipOps._chk), ``ptr(tensor)`` yields the device address -- both injectable so that tools and CPU tests can fill
    the struct for shape-only (meta) tensors and ask the library which kernel would serve the call (svr_gemm_kernel_class)."""
    chk = chk or (lambda t, dtype=None, name="tensor": t)
    ptr = ptr or (lambda t: t.data_ptr())
    chk(A, BF16, "A"); chk(W, BF16, "W")
    # ``out_f32``: the caller expects a wide store (fp32, or h16 when ``out`` is a torch.float16 tensor); the kind itself comes
    # from out.dtype
    okind = store_kind(out)
    if bool(out_f32) != (okind != STORE_BF16):
        raise ValueError(f"out must be {'fp32 / h16' if out_f32 else 'bf16'}, got {out.dtype}")
    chk(out, None, "out")
    if W.shape[1] != K or W.shape[0] < N or W.shape[0] % 128:
        raise ValueError(f"packed weight shape {tuple(W.shape)} incompatible with N={N}, K={K}")
    a = hip_lib.GemmArgs()
    if conv is not None:
        M = conv.To * conv.Ho * conv.Wo
        g = a.conv
        g.enabled = 1
        g.T, g.H, g.W, g.Cin = conv.T, conv.H, conv.W, conv.Cin
        g.To, g.Ho, g.Wo = conv.To, conv.Ho, conv.Wo
        g.kt, g.kh, g.kw = conv.k
        g.st, g.sh, g.sw = conv.stride
        g.pt, g.ph, g.pw = conv.pad
        if conv.halo is not None:
            chk(conv.halo, BF16, "halo")
            g.halo_frames = conv.halo.shape[0]
            g.halo = ptr(conv.halo)
        g.zeros = zeros_ptr
        if A.numel() != conv.T * conv.H * conv.W * conv.Cin:
            raise ValueError("conv input size mismatch")
        lda = 0
    else:
        if M is None:
            M = A.shape[0]
        if lda is None:
            lda = A.stride(0) if A.dim() == 2 else K
    if phase is not None:
        if conv is None or ps is not None or resid is not None:
            raise ValueError("phase scatter: conv mode only, without pixel shuffle / residual; fused statistics through gn_shared")
        if out.numel() < ((conv.To - 1) * phase.t_stride + 1) * 4 * conv.Ho * conv.Wo * N or not out.is_contiguous():
            raise ValueError("phase scatter: out must be the dense [frames, 2*Ho, 2*Wo, N] tensor from the launch's first frame on")
        a.phase.enabled, a.phase.py, a.phase.px, a.phase.t_stride = 1, int(phase.py), int(phase.px), int(phase.t_stride)
        if phase.quad is not None:
            if len(phase.quad) != 4 or sorted((q[0], q[1]) for q in phase.quad) != [(0, 0), (0, 1), (1, 0), (1, 1)]:
                raise ValueError("phase scatter: quad needs the four phases (0,0) (0,1) (1,0) (1,1)")
            a.phase.quad = 1
            for qpy, qpx, qw, qb, qbb, qfrag in phase.quad:
                i = 2 * int(qpy) + int(qpx)
                if qfrag is None or qfrag.numel() < N * K or (qbb is not None and tuple(qbb.shape) != (3, N)):
                    raise ValueError("phase scatter: every quad phase needs its fragment-ordered weights (and a [3, N] border bias)")
                a.phase.W_frag4[i] = ptr(chk(qfrag, BF16, "W_frag"))
                a.phase.bias4[i] = None if qb is None else ptr(chk(qb, torch.float32, "bias"))
                a.phase.bias_border4[i] = None if qbb is None else ptr(chk(qbb, torch.float32, "bias_border"))
        if phase.bias_border is not None:
            if tuple(phase.bias_border.shape) != (3, N):
                raise ValueError("phase scatter: bias_border must be [3, N]")
            a.phase.bias_border = ptr(chk(phase.bias_border, torch.float32, "bias_border"))
        ldc = 0
    if ps is not None:
        a.ps.enabled = 1
        a.ps.F, a.ps.H, a.ps.W, a.ps.rz, a.ps.C = ps.F, ps.H, ps.W, ps.rz, ps.C
        a.ps.drop_first = int(ps.drop_first)
        ldc = 0
    elif ldc is None:
        ldc = out.stride(0) if out.dim() == 2 else (N // 2 if epilogue == EPI_SWIGLU else N)
    a.A, a.lda, a.W, a.C, a.ldc = ptr(A), lda, ptr(W), ptr(out), ldc
    a.M, a.N, a.K = M, N, K
    if bias is not None:
        a.bias = ptr(chk(bias, torch.float32, "bias"))
    if gate is not None:
        a.gate = ptr(chk(gate, torch.float32, "gate"))
    if resid is not None:
        chk(resid, None, "resid")
        a.resid = ptr(resid)
        a.resid_f32 = store_kind(resid)
        a.ldr = ldr if ldr is not None else (resid.stride(0) if resid.dim() == 2 else N)
    a.epilogue, a.out_f32 = epilogue, okind
    if W_frag is not None:
        if W_frag.numel() < N * K:
            raise ValueError(f"W_frag holds {W_frag.numel()} elements, the problem needs N * K = {N * K}")
        a.W_frag = ptr(chk(W_frag, BF16, "W_frag"))
    return a, M


class HipOps:
    """The product backend.  One instance per device."""

    name = "hip"
    act_dtype = BF16          # storage dtype of activations
    phase_quad = True         # gemm(phase=PhaseScatter(quad=[...])): the four phases of a sub-pixel upsampler in one launch

    def __init__(self, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise hip_lib.HipLibraryError("HipOps needs a ROCm GPU device (cuda:N); there is no CPU fallback")
        self.lib = hip_lib.lib()          # raises loudly if the .so is not built
        with torch.cuda.device(self.device):
            buf = C.create_string_buffer(256)
            rc = self.lib.svr_device_info(buf, 256)
            self.device_info = buf.value.decode()
            if rc != 0:
                raise hip_lib.HipLibraryError(f"unsupported device: {self.device_info}")
        self.zeros = torch.zeros(64, dtype=torch.uint8, device=self.device)
        self.record_kernel_class, self.last_kernel_class = False, None

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _launch(self, name, *args):
        """An entry point that takes the stream last: called on the current stream, its status checked under its own name."""
        hip_lib.check(getattr(self.lib, name)(*args, self._stream()), name)

    def _chk(self, t, dtype=None, name="tensor"):
        if not on_device(t, self.device):
            raise ValueError(f"{name} must live on {self.device}, got {t.device}")
        if dtype is not None and t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return t

    def _out(self, name, out, shape, dtype, suffix=""):
        """A result tensor: allocated where ``out`` is None, else checked -- on the device, ``dtype``, dense, exactly ``shape``."""
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        self._chk(out, dtype, f"{name}: out")
        if tuple(out.shape) != tuple(shape):
            raise ValueError(f"{name}: out must be {tuple(shape)}{suffix}, got {tuple(out.shape)}")
        return out

    def _opt(self, t, dtype, name, numel=None):
        """Optional (or small side) operand: None -> NULL, else device / dtype / contiguity (and element count) checked."""
        if t is None:
            return None
        self._chk(t, dtype, name)
        if numel is not None and t.numel() != numel:
            raise ValueError(f"{name} must hold {numel} elements, got {tuple(t.shape)}")
        return C.c_void_p(t.data_ptr())

    def mfma_calibrate(self, seconds: float = 0.25, reps: int = 3) -> float:
        """Measurement aid (svr_mfma_calibrate; never on the data path): TFLOP/s of a bare MFMA loop on this device right now =
        the matrix-pipe rate its power limit allows.  A short launch sizes the iteration count for ``seconds``, then the median of
        ``reps`` launches timed with events on the current stream is returned."""
        with torch.cuda.device(self.device):
            ws = torch.empty(int(self.lib.svr_mfma_calibrate_workspace_bytes()), dtype=torch.uint8, device=self.device)
            flops = C.c_double(0.0)

            def run(iters):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                self._launch("svr_mfma_calibrate", C.c_void_p(ws.data_ptr()), int(iters), C.byref(flops))
                e.record()
                e.synchronize()
                return flops.value / (s.elapsed_time(e) * 1e-3) / 1e12

            run(2000)                                            # (first launch: code-object load)
            rate = run(20000)
            iters = max(2000, int(20000 * seconds / (flops.value / (rate * 1e12))))
            return sorted(run(iters) for _ in range(reps))[reps // 2]

    def set_option(self, key: str, value: int):
        """Tuning / measurement knob of the library (see svr_set_option in include/seedvr2_hip.h)."""
        hip_lib.check(self.lib.svr_set_option(key.encode(), int(value)), "svr_set_option")
        hip_lib.OPTIONS[key] = int(value)

    def empty(self, *shape, dtype=None):
        return torch.empty(*shape, dtype=dtype or BF16, device=self.device)

    # ------------------------------------------------------------------ GEMM / conv
    def pack_conv_frag(self, W, kt: int, Cin: int, N: int, taps=(3, 3)):
        """Fragment-ordered copy of packed conv weights W [Npad, kt*kh*kw*Cin] for gemm(..., W_frag=) (3x3 spatial taps for
        the LDS-halo kernel, 2x2 for the sub-pixel upsampler kernel; stride 1, Cin % 32 == 0, N % 128 == 0); None when the
        geometry is not served by those kernels."""
        kh, kw = taps
        if Cin % 64 or N % 128 or W.shape[1] != kt * kh * kw * Cin or (kh, kw) not in ((3, 3), (2, 2)):
            return None
        self._chk(W, BF16, "W")
        out = torch.empty(N * W.shape[1], dtype=BF16, device=self.device)
        self._launch("svr_conv_pack_frag_taps", _ptr(W), _ptr(out), N, W.shape[1], kt, kh, kw, Cin)
        return out

    def pack_gemm_frag(self, W):
        """Fragment-ordered copy of a packed plain-GEMM weight W [Npad, K] for gemm(..., W_frag=): the persistent GEMM kernel then
        streams the weights straight into registers and only the activations pass through LDS (csrc/svr_gemm_w4r.hip; same bits).
        None for shapes that kernel never serves (it wants whole 256-column tiles and at least two 64-wide K tiles)."""
        n, k = W.shape
        if n % 256 or k % 64 or k < 128:
            return None
        self._chk(W, BF16, "W")
        out = torch.empty(n * k, dtype=BF16, device=self.device)
        self._launch("svr_gemm_pack_frag", _ptr(W), _ptr(out), n, k)
        return out

    def gemm(self, A, W, out, *, N, K, M=None, bias=None, epilogue=EPI_BIAS, gate=None, resid=None,
             out_f32=False, conv: Optional[Conv3dGeom] = None, ps: Optional[PixelShuffleGeom] = None,
             lda=None, ldc=None, ldr=None, gn_groups: int = 0, W_frag=None, phase: Optional[PhaseScatter] = None,
             gn_shared: Optional[dict] = None):
        """out[M, N] = A[M, K] @ W[:N, :K]^T with fused epilogue.  W is [Npad, K] bf16 (Npad % 128 == 0).
        With ``gn_groups`` > 0 (conv mode) returns ``(out, stats)``: per-frame GroupNorm (sum, sumsq) of the stored
        output [To, groups, 2] fp64 fused into the conv epilogue, or ``None`` when the kernel serving this
        geometry does not produce them (the caller then runs groupnorm_stats).
        ``gn_shared`` (with ``gn_groups``): several launches write ONE output tensor (the phases of a sub-pixel upsampler); the
        caller passes the same dict {"frames": output frames, "frame0": first output frame of this launch} to each of them and
        calls gn_shared_stats() after the last -- the launches then return ``out`` only."""
        if phase is not None and gn_groups and gn_shared is None:
            raise ValueError("phase scatter: fused statistics through gn_shared")
        if phase is not None and phase.quad is not None and not self._quad_ok(A, W, out, N, K, conv, phase, out_f32):
            # the library does not take this geometry as one launch: four phase launches (same results, same order)
            import dataclasses
            for qpy, qpx, qw, qb, qbb, qfrag in sorted(phase.quad, key=lambda q: (q[0], q[1])):
                g1 = dataclasses.replace(conv, pad=(conv.pad[0], 1 - qpy, 1 - qpx))
                self.gemm(A, qw, out, N=N, K=K, bias=qb, conv=g1, phase=PhaseScatter(qpy, qpx, qbb, phase.t_stride), W_frag=qfrag,
                          out_f32=out_f32, gn_groups=gn_groups, gn_shared=gn_shared)
            return out
        a, M = fill_gemm_args(A, W, out, N=N, K=K, M=M, bias=bias, epilogue=epilogue, gate=gate, resid=resid, out_f32=out_f32,
                              conv=conv, ps=ps, lda=lda, ldc=ldc, ldr=ldr, W_frag=W_frag, phase=phase,
                              zeros_ptr=self.zeros.data_ptr(), chk=self._chk)
        stats = None
        if gn_groups > 0 and conv is not None:
            a.gn_groups = gn_groups
            nblk = int(self.lib.svr_gemm_gn_blocks(C.byref(a)))
            if gn_shared is not None:
                # one partial buffer [frames][nblk][groups] for all launches of the output tensor; a launch that cannot fuse
                # (nblk == 0, or a different block count than its siblings) switches the whole tensor back to the separate pass
                if nblk > 0 and gn_shared.get("ok", True) and gn_shared.get("nblk", nblk) == nblk:
                    if "partial" not in gn_shared:
                        gn_shared.update(nblk=nblk, groups=gn_groups, ok=True, partial=torch.empty(
                            gn_shared["frames"] * nblk * gn_groups * 2, dtype=torch.float64, device=self.device))
                    a.gn_partial = gn_shared["partial"].data_ptr() + int(gn_shared["frame0"]) * nblk * gn_groups * 16
                else:
                    gn_shared["ok"] = False
                    a.gn_groups = 0
            elif nblk > 0:
                partial = torch.empty(conv.To * nblk * gn_groups * 2, dtype=torch.float64, device=self.device)
                a.gn_partial = partial.data_ptr()
                stats = torch.empty(conv.To, gn_groups, 2, dtype=torch.float64, device=self.device)
            else:
                a.gn_groups = 0
        if self.record_kernel_class:                      # (bench.py: which kernel does the library pick for this launch)
            self.last_kernel_class = hip_lib.KERNEL_CLASSES.get(int(self.lib.svr_gemm_kernel_class(C.byref(a))), "invalid")
        self._launch("svr_gemm_bf16", C.byref(a))
        if gn_groups > 0 and gn_shared is None:
            if stats is not None:
                self._launch("svr_groupnorm_reduce", _ptr(partial), _ptr(stats), conv.To, nblk, gn_groups)
            return out, stats
        return out

    def _quad_ok(self, A, W, out, N, K, conv, phase, out_f32) -> bool:
        """Does the library serve this quad phase launch with the sub-pixel conv kernel (svr_gemm_kernel_class)?"""
        if any(q[5] is None for q in phase.quad):
            return False
        a, _ = fill_gemm_args(A, W, out, N=N, K=K, conv=conv, phase=phase, out_f32=out_f32, zeros_ptr=self.zeros.data_ptr(),
                              chk=self._chk)
        return hip_lib.KERNEL_CLASSES.get(int(self.lib.svr_gemm_kernel_class(C.byref(a)))) == "conv_subpixel"

    def gn_shared_stats(self, gn_shared: dict):
        """Statistics [frames, groups, 2] of a tensor whose launches shared ``gn_shared`` (gemm), or None when one of them could
        not fuse them (the caller then runs groupnorm_stats)."""
        if not gn_shared.get("ok", False) or "partial" not in gn_shared:
            return None
        stats = torch.empty(gn_shared["frames"], gn_shared["groups"], 2, dtype=torch.float64, device=self.device)
        self._launch("svr_groupnorm_reduce", _ptr(gn_shared["partial"]), _ptr(stats), gn_shared["frames"], gn_shared["nblk"],
                     gn_shared["groups"])
        return stats

    # ------------------------------------------------------------------ DiT side kernels
    def _xf32(self, x, name="x"):
        """activation inputs that may come from the wide residual trunk: -> the SVR_STORE_* kind (0 bf16, 1 fp32, 2 h16)"""
        self._chk(x, None, name)
        return store_kind(x)

    def rmsnorm_mod(self, x, out, eps, w=None, scale=None, shift=None):
        xf = self._xf32(x); self._chk(out, BF16, "out")
        rows, dim = x.shape
        if tuple(out.shape) != (rows, dim):
            raise ValueError("rmsnorm_mod: x must be bf16, fp32 or h16 [rows, dim] and out bf16 of the same shape")
        self._launch("svr_rmsnorm_mod", _ptr(x), _ptr(out), rows, dim, eps, self._opt(w, torch.float32, "w", dim),
                     self._opt(scale, torch.float32, "scale", dim), self._opt(shift, torch.float32, "shift", dim), xf)
        return out

    def ada_combine(self, emb, params, slots, out):
        self._chk(emb, BF16, "emb"); self._chk(params, BF16, "params")
        self._chk(slots, torch.int32, "slots"); self._chk(out, torch.float32, "out")
        n_vec, dim = params.shape
        self._launch("svr_ada_combine", _ptr(emb), _ptr(params), _ptr(slots), _ptr(out), n_vec, dim)
        return out

    def qknorm_rope(self, qkv, heads, pos, t_offset, cos_tab, sin_tab, wq, wk, eps):
        self._chk(qkv, BF16, "qkv"); self._chk(pos, torch.int16, "pos")
        self._chk(cos_tab, torch.float32, "cos_tab"); self._chk(sin_tab, torch.float32, "sin_tab")
        rows = qkv.shape[0]
        if qkv.shape[1] != 3 * heads * 128 or pos.shape != (rows, 3):
            raise ValueError("qknorm_rope: bad shapes")
        n_pos, n_freq = cos_tab.shape
        if sin_tab.shape != cos_tab.shape:
            raise ValueError("qknorm_rope: cos / sin tables of different shapes")
        if wq is None or wk is None:
            raise ValueError("qknorm_rope: the q / k norm weights are required (fp32 [128] each)")
        self._launch("svr_qknorm_rope", _ptr(qkv), rows, heads, _ptr(pos), t_offset, _ptr(cos_tab), _ptr(sin_tab), n_pos, n_freq,
                     self._opt(wq, torch.float32, "wq", 128), self._opt(wk, torch.float32, "wk", 128), eps)
        return qkv

    def attn_varlen(self, qkv, out, seq_rows, out_rows, cu, max_len, heads, head_dim, scale):
        self._chk(qkv, BF16, "qkv"); self._chk(out, BF16, "out")
        for t, n in ((seq_rows, "seq_rows"), (out_rows, "out_rows"), (cu, "cu")):
            self._chk(t, torch.int32, n)
        if qkv.dim() != 2 or out.dim() != 2 or qkv.shape[1] != 3 * heads * head_dim or out.shape[1] != heads * head_dim or \
                seq_rows.numel() != out_rows.numel() or cu.numel() < 1:
            raise ValueError("attn_varlen: qkv [rows, 3 * heads * head_dim], out [rows', heads * head_dim], one out_row per seq_row")
        self._launch("svr_attn_varlen", _ptr(qkv), qkv.stride(0), _ptr(out), out.stride(0), _ptr(seq_rows), _ptr(out_rows), _ptr(cu),
                     cu.numel() - 1, max_len, heads, head_dim, scale)
        return out

    def softmax_rows(self, S, P, scale):
        """P[r] = softmax(scale * S[r]); S fp32 [rows, cols], P bf16 [rows, cols]."""
        self._chk(S, torch.float32, "S"); self._chk(P, BF16, "P")
        rows, cols = S.shape
        self._launch("svr_softmax_rows", _ptr(S), _ptr(P), rows, cols, S.stride(0), P.stride(0), scale)
        return P

    def rows_mean(self, src, dst, n_groups, rows_per_group):
        self._chk(src, BF16, "src"); self._chk(dst, BF16, "dst")
        if src.numel() != n_groups * rows_per_group * src.shape[-1] or dst.numel() != rows_per_group * src.shape[-1]:
            raise ValueError("rows_mean: src [n_groups * rows_per_group, dim], dst [rows_per_group, dim]")
        self._launch("svr_rows_mean", _ptr(src), _ptr(dst), n_groups, rows_per_group, src.shape[-1])
        return dst

    def patchify(self, vid, out):
        self._chk(vid, BF16, "vid"); self._chk(out, BF16, "out")
        T, H, W, Cc = vid.shape
        self._launch("svr_patchify", _ptr(vid), _ptr(out), T, H, W, Cc, out.shape[1])
        return out

    def unpatchify_euler(self, pred, x_t, out):
        self._chk(pred, BF16, "pred"); self._chk(out, BF16, "out")
        T, H, W, Cc = out.shape
        if x_t is not None:
            self._chk(x_t, BF16, "x_t")
        self._launch("svr_unpatchify_euler", _ptr(pred), pred.stride(0), _ptr(x_t), _ptr(out), T, H, W, Cc)
        return out

    # ------------------------------------------------------------------ VAE side kernels
    def groupnorm_stats(self, x, stats, groups):
        xf = self._xf32(x); self._chk(stats, torch.float64, "stats")
        T, H, W, Cc = x.shape
        if stats.numel() != T * groups * 2:
            raise ValueError("groupnorm_stats: stats must be [T, groups, 2]")
        ws = torch.empty(int(self.lib.svr_groupnorm_workspace_bytes(T, H * W, groups)), dtype=torch.uint8,
                         device=self.device)
        self._launch("svr_groupnorm_stats", _ptr(x), _ptr(stats), _ptr(ws), T, H * W, Cc, groups, xf)
        return stats

    def groupnorm_apply(self, x, out, stats, gamma, beta, groups, eps, silu):
        xf = self._xf32(x); self._chk(out, BF16, "out")
        T, H, W, Cc = x.shape
        if out.numel() != x.numel():
            raise ValueError("groupnorm_apply: out must have x's shape")
        if stats is None or gamma is None or beta is None:
            raise ValueError("groupnorm_apply: stats, gamma and beta are required")
        self._launch("svr_groupnorm_apply", _ptr(x), _ptr(out), self._opt(stats, torch.float64, "stats", T * groups * 2),
                     self._opt(gamma, torch.float32, "gamma", Cc), self._opt(beta, torch.float32, "beta", Cc), T, H * W, Cc, groups,
                     eps, int(silu), xf)
        return out

    def im2col_causal(self, x, out, conv: Conv3dGeom):
        self._chk(x, BF16, "x"); self._chk(out, BF16, "out")
        g = hip_lib.ConvGeom()
        g.enabled = 1
        g.T, g.H, g.W, g.Cin = conv.T, conv.H, conv.W, conv.Cin
        g.To, g.Ho, g.Wo = conv.To, conv.Ho, conv.Wo
        g.kt, g.kh, g.kw = conv.k
        g.st, g.sh, g.sw = conv.stride
        g.pt, g.ph, g.pw = conv.pad
        if conv.halo is not None:
            g.halo_frames = conv.halo.shape[0]
            g.halo = self._chk(conv.halo, BF16, "halo").data_ptr()
        g.zeros = self.zeros.data_ptr()
        self._launch("svr_im2col_causal", _ptr(x), _ptr(out), C.byref(g), out.shape[1])
        return out

    def blend_accumulate(self, tile, acc, cnt, wy, wx, y0, x0):
        self._chk(tile, BF16, "tile"); self._chk(acc, torch.float32, "acc"); self._chk(cnt, torch.float32, "cnt")
        T, h, w, Cc = tile.shape
        Ta, H, W, Ca = acc.shape
        if (Ta, Ca) != (T, Cc) or cnt.numel() != H * W:
            raise ValueError("blend_accumulate: acc [T, H, W, C] for tile [T, h, w, C], cnt [H, W]")
        self._launch("svr_blend_accumulate", _ptr(tile), _ptr(acc), _ptr(cnt), self._opt(wy, torch.float32, "wy", h),
                     self._opt(wx, torch.float32, "wx", w), T, h, w, Cc, H, W, y0, x0)

    def blend_finalize(self, acc, cnt, out, scale=1.0, shift=0.0):
        self._chk(acc, torch.float32, "acc"); self._chk(out, BF16, "out")
        T, H, W, Cc = acc.shape
        self._chk(cnt, torch.float32, "cnt")
        if cnt.numel() != H * W or out.numel() != T * H * W * out.shape[-1]:
            raise ValueError("blend_finalize: cnt [H, W], out [T, H, W, c_take]")
        self._launch("svr_blend_finalize", _ptr(acc), _ptr(cnt), _ptr(out), T, H * W, Cc, out.shape[-1], scale, shift)
        return out

    def affine_slice(self, inp, out, scale=1.0, shift=0.0):
        self._chk(inp, BF16, "inp"); self._chk(out, BF16, "out")
        c_in, c_out = inp.shape[-1], out.shape[-1]
        rows = inp.numel() // c_in
        self._launch("svr_affine_slice", _ptr(inp), _ptr(out), rows, c_in, c_out, scale, shift)
        return out

    # ------------------------------------------------------------------ alpha channel
    def alpha_upscale(self, rgb_thwc, alpha_lo, out=None, base=None, edge_out=None):
        """Edge-guided alpha upscaling (alpha.py is the specification; csrc/svr_alpha.hip): rgb [T, H, W, >= 3] fp32 / bf16, the
        upscaled frames of ONE batch as the decoder left them (pixel stride taken as is), alpha_lo [T, h, w] -> fp32 [T, H, W].
        The bicubic base is torch glue on the device (``base``: a precomputed one); three launches on the current stream, no host
        synchronisation.  ``edge_out``: optional uint8 [T, H, W] receiving the edge bytes."""
        from . import alpha as alpha_mod
        if rgb_thwc.dim() != 4 or rgb_thwc.shape[-1] < 3 or rgb_thwc.dtype not in (torch.float32, BF16):
            raise ValueError("alpha_upscale: rgb must be [T, H, W, >= 3] in fp32 or bf16")
        T, H, W, _ = rgb_thwc.shape
        ld = rgb_thwc.stride(2)
        if rgb_thwc.device.type != "cuda" or rgb_thwc.stride(3) != 1 or ld < 3 or rgb_thwc.stride(1) != W * ld or \
                rgb_thwc.stride(0) != H * W * ld:
            raise ValueError("alpha_upscale: rgb must live on the device with dense frames (channel-last, any pixel stride >= 3)")
        if alpha_lo.dim() != 3 or alpha_lo.shape[0] != T:
            raise ValueError("alpha_upscale: alpha_lo must be [T, h, w] with rgb's frame count")
        alpha_lo = self._chk(alpha_lo.to(device=rgb_thwc.device, dtype=torch.float32).contiguous(), torch.float32, "alpha_lo")
        if base is None:
            base = alpha_mod.bicubic_base(alpha_lo, H, W)
        base = self._chk(base.contiguous(), torch.float32, "base")
        if tuple(base.shape) != (T, H, W):
            raise ValueError("alpha_upscale: base must be [T, H, W]")
        if out is None:
            out = torch.empty(T, H, W, dtype=torch.float32, device=self.device)
        self._chk(out, torch.float32, "out")
        if tuple(out.shape) != (T, H, W):
            raise ValueError("alpha_upscale: out must be [T, H, W]")
        if edge_out is not None:
            self._chk(edge_out, torch.uint8, "edge_out")
            if tuple(edge_out.shape) != (T, H, W):
                raise ValueError("alpha_upscale: edge_out must be [T, H, W]")
        kind = 1 if rgb_thwc.dtype == torch.float32 else 0                   # SVR_STORE_FP32 / SVR_STORE_BF16
        nbytes = int(self.lib.svr_alpha_workspace_bytes(T, H, W))
        if nbytes <= 0:
            raise ValueError("alpha_upscale: need T >= 1 and frames of at least 2 x 2 pixels")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        rgb_p, ws_p, n_alpha = _ptr(rgb_thwc), _ptr(ws), alpha_lo.numel()
        self._launch("svr_alpha_stats", _ptr(alpha_lo), n_alpha, rgb_p, T, H, W, ld, kind, ws_p, nbytes)
        self._launch("svr_alpha_edges", rgb_p, T, H, W, ld, kind, ws_p, nbytes)
        self._launch("svr_alpha_refine", rgb_p, _ptr(base), _ptr(out), self._opt(edge_out, torch.uint8, "edge_out"), T, H, W, ld, kind,
                     n_alpha, ws_p, nbytes)
        return out

    # ------------------------------------------------------------------ packed output frames
    def _pack_args(self, name, frames, fmt, out, colour=None, planes=None):
        """What pack_frames, pack_yuv420p10 and pack_planar check before their launch -> (T, H, W, Cn, x_kind, out); ``out`` allocated
        where it was None.  ``colour``: pack_yuv420p10's (matrix, range_, siting), refused with the format.  ``planes``: pack_planar's
        (sub, bits, matrix, range_, siting) in place of a format."""
        from . import frameio, planar, planar_out

        def codes_and_channels(T, H, W, Cn):                   # (the format judges the channel count)
            try:
                if planes is not None:
                    planar_out.check_arguments(*planes)
                    return planar_out.check_channels(Cn)
                if colour is not None:
                    frameio.check_colour(*colour)
                frameio.packed_shape(T, H, W, Cn, fmt)
            except ValueError as e:
                return str(e)

        T, H, W, Cn, kind = clip_args(name, frames, self.device, channels=None, before=codes_and_channels)
        if planes is not None:
            return T, H, W, Cn, kind, self._out(name, out, planar.planar_shape(T, H, W, planes[0]), planar.planar_dtype(planes[1]))
        out = self._out(name, out, frameio.packed_shape(T, H, W, Cn, fmt), frameio.packed_dtype(fmt), suffix="" if colour else f" for {fmt}")
        return T, H, W, Cn, kind, out

    def pack_frames(self, frames, fmt, out=None):
        """Output frames narrowed on the device (frameio.py is the specification; csrc/svr_frame_pack.hip, yuv420p10 through
        csrc/svr_frame_pack_colour.hip): frames [T, H, W, 3 | 4] fp32 / bf16, dense -> uint8 [T, H, W, C] ("rgb8", "bgr8") or
        uint16 [T, H*W + 2*h2*w2] ("yuv420p10", C = 3).  One launch on the current stream, no host synchronisation.  ``out``: a dense
        tensor of exactly that shape and dtype."""
        T, H, W, Cn, kind, out = self._pack_args("pack_frames", frames, fmt, out)
        self._launch("svr_pack_frames", _ptr(frames), kind, T, H, W, Cn, hip_lib.PACK_FORMATS[fmt], _ptr(out),
                     out.numel() * out.element_size())
        return out

    def pack_yuv420p10(self, frames, matrix="bt709", range_="tv", siting="center", out=None):
        """yuv420p10 planes with a chosen matrix ("bt709" | "bt601" | "bt2020"), range ("tv" | "pc") and chroma siting ("center" |
        "left") on the device (frameio.pack_yuv420p10_torch is the specification; csrc/svr_frame_pack_colour.hip): frames
        [T, H, W, 3] fp32 / bf16, dense -> uint16 [T, H*W + 2*h2*w2].  One launch on the current stream, no host synchronisation.
        ``out``: a dense tensor of exactly that shape and dtype."""
        T, H, W, _, kind, out = self._pack_args("pack_yuv420p10", frames, "yuv420p10", out, colour=(matrix, range_, siting))
        self._launch("svr_pack_yuv420p10", _ptr(frames), kind, T, H, W, hip_lib.COLOUR_MATRICES[matrix], hip_lib.COLOUR_RANGES[range_],
                     hip_lib.COLOUR_SITINGS[siting], _ptr(out), out.numel() * out.element_size())
        return out

    def pack_planar(self, frames, sub, bits, matrix="bt709", range_="tv", siting="left", out=None):
        """Planar YUV planes of a chosen subsampling ("420" | "422" | "444"), depth (8 | 10 | 12), matrix, range and chroma siting
        ("center" | "left" | "topleft", as far as the subsampling takes them) on the device (planar_out.pack_planar_torch is the
        specification; csrc/svr_planar_out.hip): frames [T, H, W, 3] fp32 / bf16, dense -> uint8 (8 bits) or uint16
        [T, H*W + 2*hc*wc], planar.planar_shape's layout.  One launch on the current stream, no host synchronisation.  ``out``: a
        dense tensor of exactly that shape and dtype."""
        T, H, W, _, kind, out = self._pack_args("pack_planar", frames, None, out, planes=(sub, bits, matrix, range_, siting))
        self._launch("svr_pack_planar", _ptr(frames), kind, T, H, W, hip_lib.PLANAR_SUBS[sub], int(bits), hip_lib.COLOUR_MATRICES[matrix],
                     hip_lib.COLOUR_RANGES[range_], hip_lib.PLANAR_OUT_SITINGS[siting], _ptr(out), out.numel() * out.element_size())
        return out

    # ------------------------------------------------------------------ frame signatures (cut detection)
    def frame_signatures(self, frames, out=None):
        """Per frame the 4 x 4 grid of 64-bin luma histograms cut detection compares (shots.py is the specification, bit for bit;
        csrc/svr_shots.hip): frames [T, H, W, 3 | 4] fp32 / bf16, dense, H >= 4, W >= 4 -> int32 [T, 1024].  The call zeroes the
        result itself; one memset and one launch on the current stream, no host synchronisation.  ``out``: a dense int32 [T, 1024]
        tensor."""
        T, H, W, Cn, kind = clip_args("frame_signatures", frames, self.device, min_hw=4, after=lambda T, H, W, _: (
            f"frames of H * W = {H * W} pixels; the int32 counters hold fewer than 2^31" if H * W >= 1 << 31 else None))
        out = self._out("frame_signatures", out, (T, 1024), torch.int32)
        self._launch("svr_frame_signatures", _ptr(frames), kind, T, H, W, Cn, _ptr(out), out.numel() * 4)
        return out

    # ------------------------------------------------------------------ active-area profile (letterbox bars)
    def active_profile(self, frames, dark, out=None):
        """Per row and per column of a clip the number of pixels, over all frames, whose 8-bit luma exceeds ``dark`` (active.py is
        the specification, bit for bit; csrc/svr_active.hip): frames [T, H, W, 3 | 4] fp32 / bf16, dense, T * max(H, W) < 2^31,
        dark an integer in 0..255 -> int32 [H + W], rows first.  The call zeroes the result itself; one memset and one launch on
        the current stream, no host synchronisation.  ``out``: a dense int32 [H + W] tensor."""
        def counters_and_dark(T, H, W, _):
            if T * max(H, W) >= 1 << 31:
                return f"frames of T * max(H, W) = {T * max(H, W)}; the int32 counters hold fewer than 2^31"
            if isinstance(dark, bool) or not isinstance(dark, int) or not 0 <= dark <= 255:
                return f"dark must be an integer in 0..255, got {dark!r}"

        T, H, W, Cn, kind = clip_args("active_profile", frames, self.device, min_hw=1, after=counters_and_dark)
        out = self._out("active_profile", out, (H + W,), torch.int32)
        self._launch("svr_active_profile", _ptr(frames), kind, T, H, W, Cn, dark, _ptr(out), out.numel() * 4)
        return out

    # ------------------------------------------------------------------ PNG streams
    def encode_png_bytes(self, T, H, W, Cn, depth=8, runs=False):
        """-> (scratch bytes of one encode_png call, capacity in bytes of each frame's slot of ``out``) for a geometry.  The
        capacity is the same with and without ``runs``; the scratch is larger with them."""
        scratch, cap = C.c_int64(0), C.c_int64(0)
        fn = self.lib.svr_png_encode_runs_bytes if runs else self.lib.svr_png_encode_bytes
        if fn(int(T), int(H), int(W), int(Cn), int(depth), C.byref(scratch), C.byref(cap)) != 0:
            raise ValueError(f"encode_png: {self.lib.svr_last_error().decode()}")
        return scratch.value, cap.value

    def encode_png(self, frames, depth=8, out=None, sizes=None, runs=False):
        """Output frames encoded as PNG zlib streams on the device (pngenc.py is the specification, byte for byte;
        csrc/svr_png.hip): frames [T, H, W, 3 | 4] fp32 / bf16, dense, ``depth`` 8 or 16 -> (out uint8 [T, cap], sizes int64 [T]):
        frame t's stream is out[t, :sizes[t]] (pngenc.png_file frames it as a file); bytes past it are not written.  Three launches
        on the current stream, no host synchronisation.  ``out``: a dense uint8 [T, >= pngenc.frame_bound(H, W, C, depth)] tensor;
        ``sizes``: a dense int64 [T] tensor.  ``runs``: the stream with run-length matches (pngenc.encode_frames_spec(...,
        runs=True); svr_png_encode_runs, four launches) -- never longer than the literal one, and decoding to the same samples."""
        T, H, W, Cn, kind = clip_args("encode_png", frames, self.device, channels="C must be 3 or 4", before=lambda *_: (
            None if depth in (8, 16) else f"depth must be 8 or 16, got {depth}"))
        nscratch, cap = self.encode_png_bytes(T, H, W, Cn, depth, runs)
        if out is None:
            out = torch.empty((T, cap), dtype=torch.uint8, device=self.device)
        self._chk(out, torch.uint8, "encode_png: out")
        if out.dim() != 2 or out.shape[0] != T or out.shape[1] < cap:
            raise ValueError(f"encode_png: out must be uint8 [{T}, >= {cap}], got {tuple(out.shape)}")
        if sizes is None:
            sizes = torch.empty(T, dtype=torch.int64, device=self.device)
        self._chk(sizes, torch.int64, "encode_png: sizes")
        if tuple(sizes.shape) != (T,):
            raise ValueError(f"encode_png: sizes must be int64 [{T}], got {tuple(sizes.shape)}")
        scratch = torch.empty(nscratch, dtype=torch.uint8, device=self.device)
        self._launch("svr_png_encode_runs" if runs else "svr_png_encode", _ptr(frames), kind, T, H, W, Cn, int(depth), _ptr(scratch),
                     nscratch, _ptr(out), out.shape[1], _ptr(sizes))
        return out, sizes

    # ------------------------------------------------------------------ colour correction
    # (colorfix.py is the specification; csrc/svr_colorfix.hip.)  Pixel operands are fp32 [T, 3, H, W]-SHAPED tensors of any
    # strides -- the pipeline's channels-last frames and its sliced [C, T, H, W] reference are read where they lie.  A result
    # allocated here is a dense [T, H, W, 3] buffer returned as its [T, 3, H, W] view.
    def _pixels(self, t, name, shape=None, output=False):
        if t.dim() != 4 or t.shape[1] != 3 or t.dtype != torch.float32 or (shape is not None and tuple(t.shape) != tuple(shape)):
            want = "[T, 3, H, W]" if shape is None else str(tuple(shape))
            raise ValueError(f"{name} must be fp32 {want}, got {t.dtype} {tuple(t.shape)}")
        if not on_device(t, self.device):
            raise ValueError(f"{name} must live on {self.device}, got {t.device}")
        if t.numel() == 0:
            raise ValueError(f"{name} must hold at least one pixel, got {tuple(t.shape)}")
        if output and min(t.stride()) < 1:
            raise ValueError(f"{name} must not be an expanded view (strides {t.stride()})")
        return (C.c_int64 * 4)(*t.stride())

    def _pixels_out(self, out, like, name, *inputs):
        if out is None:
            T, _, H, W = like.shape
            out = torch.empty((T, H, W, 3), dtype=torch.float32, device=self.device).permute(0, 3, 1, 2)
        strides = self._pixels(out, name, like.shape, output=True)
        if any(out.untyped_storage().data_ptr() == x.untyped_storage().data_ptr() for x in inputs):
            raise ValueError(f"{name} must not share its storage with an input")
        return out, strides

    def wavelet_reconstruct(self, content, style, out=None):
        """clamp(high5(content) + low5(style), -1, 1): colorfix.wavelet_reconstruction bit for bit, in one launch."""
        cs = self._pixels(content, "wavelet_reconstruct: content")
        ss = self._pixels(style, "wavelet_reconstruct: style", content.shape)
        out, os_ = self._pixels_out(out, content, "wavelet_reconstruct: out", content, style)
        T, _, H, W = content.shape
        self._launch("svr_wavelet_reconstruct", _ptr(content), cs, _ptr(style), ss, _ptr(out), os_, T, H, W, 1)
        return out

    def lab_planes(self, base, style, c_lab=None, s_lab=None):
        """[-1, 1] frames -> CIELAB planes (colorfix.rgb_to_lab of ((x + 1) * 0.5).clamp(0, 1)): two dense fp32 [3, T*H*W]."""
        bs = self._pixels(base, "lab_planes: base")
        ss = self._pixels(style, "lab_planes: style", base.shape)
        T, _, H, W = base.shape
        planes = []
        for t, name in ((c_lab, "lab_planes: c_lab"), (s_lab, "lab_planes: s_lab")):
            if t is None:
                t = torch.empty((3, T * H * W), dtype=torch.float32, device=self.device)
            self._chk(t, torch.float32, name)
            if tuple(t.shape) != (3, T * H * W):
                raise ValueError(f"{name} must be fp32 {(3, T * H * W)}, got {tuple(t.shape)}")
            planes.append(t)
        self._launch("svr_lab_planes", _ptr(base), bs, _ptr(style), ss, _ptr(planes[0]), _ptr(planes[1]), T, H, W, 1)
        return planes[0], planes[1]

    def lab_merge(self, c_L, m_L, m_a, m_b, luminance_weight, shape, out=None):
        """L = c_L * w + m_L * (1 - w) (w >= 1: c_L alone, ``m_L`` may be None), matched a and b -> colorfix.lab_to_rgb, clamped,
        * 2 - 1.  The planes are dense fp32 [T*H*W]; ``shape`` = (T, H, W); -> [T, 3, H, W]."""
        T, H, W = (int(v) for v in shape)
        w = float(luminance_weight)
        if w >= 1.0:
            m_L = None
        elif m_L is None:
            raise ValueError("lab_merge: m_L is needed for luminance_weight < 1")
        for t, name in ((c_L, "c_L"), (m_L, "m_L"), (m_a, "m_a"), (m_b, "m_b")):
            if t is not None:
                self._chk(t, torch.float32, f"lab_merge: {name}")
                if t.numel() != T * H * W:
                    raise ValueError(f"lab_merge: {name} must hold T * H * W = {T * H * W} values, got {tuple(t.shape)}")
        like = torch.empty((T, 3, H, W), dtype=torch.float32, device="meta")
        out, os_ = self._pixels_out(out, like, "lab_merge: out")
        self._launch("svr_lab_merge", _ptr(c_L), _ptr(m_L), _ptr(m_a), _ptr(m_b), w, _ptr(out), os_, T, H, W, 1)
        return out

    def chan_stats(self, content, style, stats=None):
        """-> fp32 [T, 3, 4]: mean and unbiased variance of content, then of style, per frame and channel (fp64 sums, fixed order)."""
        cs = self._pixels(content, "chan_stats: content")
        ss = self._pixels(style, "chan_stats: style", content.shape)
        T, _, H, W = content.shape
        if stats is None:
            stats = torch.empty((T, 3, 4), dtype=torch.float32, device=self.device)
        self._chk(stats, torch.float32, "chan_stats: stats")
        if tuple(stats.shape) != (T, 3, 4):
            raise ValueError(f"chan_stats: stats must be fp32 {(T, 3, 4)}, got {tuple(stats.shape)}")
        nbytes = int(self.lib.svr_colorfix_workspace_bytes(T))
        if nbytes <= 0:
            raise ValueError(f"chan_stats: at most 21845 frames per call, got {T}")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
        self._launch("svr_chan_stats", _ptr(content), cs, _ptr(style), ss, _ptr(stats), T, H, W, 1, _ptr(ws), nbytes)
        return stats

    def adain(self, content, style, eps=1e-5, out=None):
        """colorfix.adaptive_instance_normalization: per frame and channel, content moved to the style's mean and deviation."""
        stats = self.chan_stats(content, style)
        cs = self._pixels(content, "adain: content")
        out, os_ = self._pixels_out(out, content, "adain: out")
        T, _, H, W = content.shape
        self._launch("svr_adain_apply", _ptr(content), cs, _ptr(stats), float(eps), _ptr(out), os_, T, H, W, 1)
        return out

    # (colorfix.sort_key / rank_match_spec are the specification, bit for bit; csrc/svr_rank.hip.)
    def _rank_workspace(self, n, what):
        nbytes = int(self.lib.svr_rank_workspace_bytes(n))
        if nbytes <= 0:
            raise ValueError(f"{what}: between 1 and 2^30 elements per call, got {n}")
        return torch.empty(nbytes, dtype=torch.uint8, device=self.device), nbytes

    def sort_f32(self, keys, index=True, sorted_out=None, index_out=None):
        """Stable ascending sort of an fp32 tensor (flattened), the order of ``torch.sort(stable=True)`` on the CPU with NaN last
        -> (sorted fp32 [n] of canonical values, uint32-valued int32 [n] source indices or None for ``index=False``: keys only)."""
        self._chk(keys, torch.float32, "sort_f32: keys")
        if hip_lib.OPTIONS.get("rank_launches", 3) != 3:
            raise hip_lib.HipLibraryError("sort_f32: set_option('rank_launches') is below 3 (a measurement setting under which "
                                          "svr_sort_f32 stores nothing); set it back to 3")
        n = keys.numel()
        ws, nbytes = self._rank_workspace(n, "sort_f32")

        def out(t, dtype, name):
            if t is None:
                t = torch.empty(n, dtype=dtype, device=self.device)
            self._chk(t, dtype, name)
            if t.numel() != n:
                raise ValueError(f"{name} must hold {n} elements, got {tuple(t.shape)}")
            return t

        sorted_out = out(sorted_out, torch.float32, "sort_f32: sorted_out")
        idx = out(index_out, torch.int32, "sort_f32: index_out") if index else None      # keys only: no index is allocated
        self._launch("svr_sort_f32", _ptr(keys), n, _ptr(sorted_out), _ptr(idx), _ptr(ws), nbytes)
        return sorted_out, idx

    def rank_match(self, source, reference, out=None):
        """colorfix.rank_match_spec: the k-th smallest source value becomes the k-th smallest reference value, ties to the lower
        flat index.  Two fp32 tensors of one size; ``out`` may be ``source`` itself (matched in place)."""
        self._chk(source, torch.float32, "rank_match: source")
        self._chk(reference, torch.float32, "rank_match: reference")
        n = source.numel()
        if reference.numel() != n:
            raise ValueError(f"rank_match: source and reference must hold the same number of elements, got {tuple(source.shape)} and "
                             f"{tuple(reference.shape)} (unequal sizes: colorfix.histogram_match)")
        if out is None:
            out = torch.empty_like(source)
        self._chk(out, torch.float32, "rank_match: out")
        if tuple(out.shape) != tuple(source.shape):
            raise ValueError(f"rank_match: out must be fp32 {tuple(source.shape)}, got {tuple(out.shape)}")
        ws, nbytes = self._rank_workspace(n, "rank_match")
        self._launch("svr_rank_match", _ptr(source), _ptr(reference), n, _ptr(out), _ptr(ws), nbytes)
        return out

    # (colorfix.hsv_spec / wavelet_adaptive_spec / hue_match_spec are the specification; csrc/svr_hsv.hip.)
    def _plane(self, t, n, name):
        self._chk(t, torch.float32, name)
        if t.numel() != n:
            raise ValueError(f"{name} must hold {n} values, got {tuple(t.shape)}")
        return t

    def hsv_planes(self, content, style, c_hsv=None, s_hs=None):
        """[-1, 1] frames -> colorfix.rgb_to_hsv of ((x + 1) * 0.5).clamp(0, 1), bit for bit: dense fp32 planes, content
        [3, T*H*W] (h, s, v) and style [2, T*H*W] (h, s)."""
        cs = self._pixels(content, "hsv_planes: content")
        ss = self._pixels(style, "hsv_planes: style", content.shape)
        T, _, H, W = content.shape
        planes = []
        for t, k, name in ((c_hsv, 3, "hsv_planes: c_hsv"), (s_hs, 2, "hsv_planes: s_hs")):
            if t is None:
                t = torch.empty((k, T * H * W), dtype=torch.float32, device=self.device)
            self._chk(t, torch.float32, name)
            if tuple(t.shape) != (k, T * H * W):
                raise ValueError(f"{name} must be fp32 {(k, T * H * W)}, got {tuple(t.shape)}")
            planes.append(t)
        self._launch("svr_hsv_planes", _ptr(content), cs, _ptr(style), ss, _ptr(planes[0]), _ptr(planes[1]), T, H, W, 1)
        return planes[0], planes[1]

    def hue_match(self, c_h, c_s, s_h, s_s, out=None):
        """colorfix.hue_match_spec (12 bins, more than 100 pixels on both sides), bit for bit: four fp32 planes, content and style
        each of one size; ``out`` may be ``c_s`` itself.  Reads the class counts on the host: one synchronisation of the stream."""
        n = c_s.numel()
        for t, name in ((c_h, "c_h"), (c_s, "c_s"), (s_h, "s_h"), (s_s, "s_s")):
            self._plane(t, n, f"hue_match: {name}")
        if hip_lib.OPTIONS.get("rank_launches", 3) != 3:
            raise hip_lib.HipLibraryError("hue_match: set_option('rank_launches') is below 3 (a measurement setting); set it back to 3")
        if out is None:
            out = torch.empty_like(c_s)
        self._chk(out, torch.float32, "hue_match: out")
        if tuple(out.shape) != tuple(c_s.shape):
            raise ValueError(f"hue_match: out must be fp32 {tuple(c_s.shape)}, got {tuple(out.shape)}")
        nbytes = int(self.lib.svr_hue_match_workspace_bytes(n))
        if nbytes <= 0:
            raise ValueError(f"hue_match: between 1 and 2^30 elements per plane, got {n}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self._launch("svr_hue_match", _ptr(c_h), _ptr(c_s), _ptr(s_h), _ptr(s_s), n, _ptr(out), _ptr(ws), nbytes)
        return out

    def hsv_merge(self, h, sat, v, shape, out=None):
        """colorfix.hsv_to_rgb(h, sat, v) clamped to [0, 1], * 2 - 1, bit for bit.  Dense fp32 planes [T*H*W]; ``shape`` = (T, H, W);
        -> [T, 3, H, W]."""
        T, H, W = (int(x) for x in shape)
        for t, name in ((h, "h"), (sat, "sat"), (v, "v")):
            self._plane(t, T * H * W, f"hsv_merge: {name}")
        like = torch.empty((T, 3, H, W), dtype=torch.float32, device="meta")
        out, os_ = self._pixels_out(out, like, "hsv_merge: out")
        self._launch("svr_hsv_merge", _ptr(h), _ptr(sat), _ptr(v), _ptr(out), os_, T, H, W, 1)
        return out

    def adaptive_blend(self, base, content, style, h, sat, v, threshold=0.15, sharpness=5.0, out=None):
        """The blend of colorfix.wavelet_adaptive_color_correction: ``base`` (the wavelet result) and the HSV pixel of (h, sat, v)
        mixed by w = sigmoid(sharpness * (sat(content) - sat(style) - threshold)), gated by sat(base) - sat(style) > threshold / 2."""
        bs = self._pixels(base, "adaptive_blend: base")
        cs = self._pixels(content, "adaptive_blend: content", base.shape)
        ss = self._pixels(style, "adaptive_blend: style", base.shape)
        T, _, H, W = base.shape
        for t, name in ((h, "h"), (sat, "sat"), (v, "v")):
            self._plane(t, T * H * W, f"adaptive_blend: {name}")
        out, os_ = self._pixels_out(out, base, "adaptive_blend: out", base, content, style)
        self._launch("svr_adaptive_blend", _ptr(base), bs, _ptr(content), cs, _ptr(style), ss, _ptr(h), _ptr(sat), _ptr(v),
                     float(threshold), float(sharpness), _ptr(out), os_, T, H, W, 1)
        return out

    # ------------------------------------------------------------------ packed input frames
    def unpack_frames(self, packed, fmt, T, H, W, C, matrix="bt709", range_="tv", out=None):
        """Input frames widened on the device (frameio_in.py is the specification; csrc/svr_frame_unpack.hip): ``packed`` a dense
        uint8 ("rgb8", "bgr8", "yuv420p8") or uint16 ("rgb16", "yuv420p10") tensor of exactly the format's samples -> fp32
        [T, H, W, C].  One launch on the current stream, no host synchronisation.  ``out``: a dense fp32 tensor of that shape."""
        from . import frameio_in
        try:
            frameio_in.check_arguments(packed, fmt, T, H, W, C, matrix, range_)
        except ValueError as e:
            raise ValueError(f"unpack_frames: {e}") from None
        self._chk(packed, None, "unpack_frames: packed")
        out = self._out("unpack_frames", out, (T, H, W, C), torch.float32)
        self._launch("svr_unpack_frames", _ptr(packed), packed.numel() * packed.element_size(), hip_lib.UNPACK_FORMATS[fmt], T, H, W, C,
                     hip_lib.YUV_MATRICES[matrix], hip_lib.YUV_RANGES[range_], _ptr(out), out.numel() * out.element_size())
        return out

    # ------------------------------------------------------------------ planar YUV sources
    def planar_codes(self, planes, sub, bits, T, H, W, matrix="bt709", range_="tv", siting="left", out=None):
        """Planar YUV turned into rgb16 codes on the device (planar.py is the specification; csrc/svr_planar.hip): ``planes`` a dense
        uint8 (8 bits) or uint16 (10 / 12 bits) tensor of exactly the format's samples, ``sub`` "420" | "422" | "444" -> uint16
        [T, H, W, 3], unpack_frames' "rgb16".  One launch on the current stream, no host synchronisation.  ``out``: a dense uint16
        tensor of that shape, apart from ``planes``."""
        from . import planar
        try:
            planar.check_arguments(planes, sub, bits, T, H, W, matrix, range_, siting)
        except ValueError as e:
            raise ValueError(f"planar_codes: {e}") from None
        self._chk(planes, None, "planar_codes: planes")
        out = self._out("planar_codes", out, (T, H, W, 3), torch.uint16)
        self._launch("svr_planar_codes", _ptr(planes), planes.numel() * planes.element_size(), hip_lib.PLANAR_SUBS[sub], int(bits), T, H, W,
                     hip_lib.COLOUR_MATRICES[matrix], hip_lib.COLOUR_RANGES[range_], hip_lib.PLANAR_SITINGS[siting], _ptr(out),
                     out.numel() * out.element_size())
        return out

    # ------------------------------------------------------------------ interlaced sources
    def deinterlace(self, packed, fmt, T, H, W, C, order, rate, before=None, after=None, out=None):
        """Woven frames made progressive on the packed planes (deinterlace.py is the specification; csrc/svr_deinterlace.hip):
        ``packed`` as unpack_frames takes it, ``order`` "tff" | "bff", ``rate`` "frame" | "field", ``before`` / ``after`` one packed
        frame each or None (the clip is mirrored at that end) -> T or 2 T frames in the same dtype and layout.  One launch per plane
        on the current stream, no host synchronisation.  ``out``: a dense tensor of exactly that shape and dtype, apart from every
        input."""
        from . import deinterlace
        try:
            shape = deinterlace.check_arguments(packed, fmt, T, H, W, C, order, rate, before, after)
        except ValueError as e:
            raise ValueError(f"deinterlace: {e}") from None
        self._chk(packed, None, "deinterlace: packed")
        for name, frame in (("before", before), ("after", after)):
            if frame is not None:
                self._chk(frame, None, f"deinterlace: {name}")
        n_out = T * (2 if rate == "field" else 1)
        out = self._out("deinterlace", out, (n_out,) + tuple(shape[1:]), packed.dtype)
        self._launch("svr_deinterlace", _ptr(packed), packed.numel() * packed.element_size(), _ptr(before), _ptr(after),
                     hip_lib.UNPACK_FORMATS[fmt], T, H, W, C, hip_lib.FIELD_ORDERS[order], hip_lib.DEINT_RATES[rate], _ptr(out),
                     out.numel() * out.element_size())
        return out

    # ------------------------------------------------------------------ field matching
    def comb_counts(self, packed, fmt, T, H, W, C, order, thr, before=None, after=None, out=None):
        """Per frame the combing of the three weaves its kept field can make (fieldmatch.py is the specification;
        csrc/svr_fieldmatch.hip): ``packed``, ``before`` / ``after`` and ``order`` as deinterlace takes them, ``thr`` in 0..255 ->
        int32 [T, 3, 2]: (total, peak) of the candidates cur, prev, next.  The counts are zeroed and one kernel is launched on the
        current stream, no host synchronisation.  ``out``: a dense int32 [T, 3, 2] tensor apart from every input."""
        from . import fieldmatch
        try:
            fieldmatch.check_arguments(packed, fmt, T, H, W, C, order, thr, before, after)
        except ValueError as e:
            raise ValueError(f"comb_counts: {e}") from None
        self._chk(packed, None, "comb_counts: packed")
        for name, frame in (("before", before), ("after", after)):
            if frame is not None:
                self._chk(frame, None, f"comb_counts: {name}")
        out = self._out("comb_counts", out, (T, 3, 2), torch.int32)
        self._launch("svr_comb_counts", _ptr(packed), packed.numel() * packed.element_size(), _ptr(before), _ptr(after),
                     hip_lib.UNPACK_FORMATS[fmt], T, H, W, C, hip_lib.FIELD_ORDERS[order], thr, _ptr(out), out.numel() * 4)
        return out

    def field_select(self, packed, deint, cnt, fmt, T, H, W, C, order, mi, before=None, after=None, out=None, modes=None, stats=None):
        """The progressive frames field matching chooses (fieldmatch.select_torch of fieldmatch.modes_torch(cnt, mi, s);
        csrc/svr_fieldmatch.hip): ``deint`` the clip deinterlaced at rate "frame", ``cnt`` comb_counts' int32 [T, 3, 2], both read on
        the device in stream order; ``mi`` >= 0 -> T frames in packed's dtype and layout.  ``modes`` int32 [T] receives the modes,
        ``stats`` int64 [6] (fieldmatch.Stats.counts) is added to; both may be None.  One launch per plane on the current stream, no
        host synchronisation.  ``out``: a dense tensor of packed's shape and dtype, apart from every input."""
        from . import deinterlace, fieldmatch
        try:
            shape = deinterlace.check_arguments(packed, fmt, T, H, W, C, order, "frame", before, after)
            fieldmatch.check_mi(mi)
        except ValueError as e:
            raise ValueError(f"field_select: {e}") from None
        self._chk(packed, None, "field_select: packed")
        for name, frame in (("before", before), ("after", after)):
            if frame is not None:
                self._chk(frame, None, f"field_select: {name}")
        self._chk(deint, packed.dtype, "field_select: deint")
        if deint.numel() != packed.numel():
            raise ValueError(f"field_select: deint must hold the {packed.numel()} samples of packed, got {tuple(deint.shape)}")
        self._chk(cnt, torch.int32, "field_select: cnt")
        if tuple(cnt.shape) != (T, 3, 2):
            raise ValueError(f"field_select: cnt must be {(T, 3, 2)}, got {tuple(cnt.shape)}")
        out = self._out("field_select", out, tuple(shape), packed.dtype)
        self._launch("svr_field_select", _ptr(packed), packed.numel() * packed.element_size(), _ptr(before), _ptr(after), _ptr(deint),
                     deint.numel() * deint.element_size(), _ptr(cnt), cnt.numel() * 4, hip_lib.UNPACK_FORMATS[fmt], T, H, W, C,
                     hip_lib.FIELD_ORDERS[order], mi, _ptr(out), out.numel() * out.element_size(),
                     self._opt(modes, torch.int32, "field_select: modes", T), self._opt(stats, torch.int64, "field_select: stats", 6))
        return out

    # ------------------------------------------------------------------ decimation
    def frame_diffs(self, packed, fmt, T, H, W, C, before=None, out=None):
        """Per frame the largest 32 x 32 block sum of its absolute difference from the frame before it, on plane 0 (decimate.py is the
        specification; csrc/svr_decimate.hip): ``packed`` as deinterlace takes it, ``before`` one packed frame or None (diff[0] is
        then 2^31 - 1) -> int32 [T].  The diffs are zeroed and one kernel is launched on the current stream, no host
        synchronisation.  ``out``: a dense int32 [T] tensor apart from every input."""
        from . import decimate
        try:
            decimate.check_arguments(packed, fmt, T, H, W, C, before=before)
        except ValueError as e:
            raise ValueError(f"frame_diffs: {e}") from None
        self._chk(packed, None, "frame_diffs: packed")
        if before is not None:
            self._chk(before, None, "frame_diffs: before")
        out = self._out("frame_diffs", out, (T,), torch.int32)
        self._launch("svr_frame_diffs", _ptr(packed), packed.numel() * packed.element_size(), _ptr(before), hip_lib.UNPACK_FORMATS[fmt],
                     T, H, W, C, _ptr(out), out.numel() * 4)
        return out

    def decimate_select(self, packed, diff, fmt, T, H, W, C, dup, out=None, drops=None, stats=None):
        """The frames decimation keeps (decimate.select_torch of decimate.drops_torch(diff); csrc/svr_decimate.hip): ``diff``
        frame_diffs' int32 [T], read on the device in stream order; ``dup`` in 0..2^18 -> T - T // 5 frames in packed's dtype and
        layout.  ``drops`` int32 [T // 5] receives the dropped positions, ``stats`` int64 [6] (decimate.Stats.counts) is added to;
        both may be None.  One launch on the current stream, no host synchronisation.  ``out``: a dense tensor of that shape and
        packed's dtype, apart from every input."""
        from . import decimate
        try:
            shape = decimate.check_arguments(packed, fmt, T, H, W, C, dup)
        except ValueError as e:
            raise ValueError(f"decimate_select: {e}") from None
        self._chk(packed, None, "decimate_select: packed")
        self._chk(diff, torch.int32, "decimate_select: diff")
        if tuple(diff.shape) != (T,):
            raise ValueError(f"decimate_select: diff must be {(T,)}, got {tuple(diff.shape)}")
        out = self._out("decimate_select", out, (T - T // decimate.CYCLE,) + tuple(shape[1:]), packed.dtype)
        self._launch("svr_decimate_select", _ptr(packed), packed.numel() * packed.element_size(), _ptr(diff), diff.numel() * 4,
                     hip_lib.UNPACK_FORMATS[fmt], T, H, W, C, dup, _ptr(out), out.numel() * out.element_size(),
                     self._opt(drops, torch.int32, "decimate_select: drops", T // decimate.CYCLE),
                     self._opt(stats, torch.int64, "decimate_select: stats", 6))
        return out

    # ------------------------------------------------------------------ GGUF blocks expanded at load
    def dequant_gguf(self, blocks, ggml_type, out_dtype=BF16, out=None):
        """GGUF blocks expanded on the device (gguf.py is the specification, bit for bit; csrc/svr_gguf.hip): ``blocks`` a dense uint8
        tensor of whole Q8_0 / Q4_K / Q5_K / Q6_K blocks (a storage-offset view is fine; one that does not start on 32 bytes -- GGUF's
        own alignment makes that the rare case -- is copied to a fresh allocation first) -> [n_blocks, block size] bf16 or fp32.  One
        launch on the current stream, no host synchronisation.  ``out``: a dense tensor of exactly that shape and dtype."""
        from . import gguf
        if ggml_type not in gguf.QUANTISED:
            raise ValueError(f"dequant_gguf: unsupported ggml type {gguf.type_name(ggml_type)}")
        if out_dtype not in (BF16, torch.float32):
            raise ValueError(f"dequant_gguf: out_dtype must be torch.bfloat16 or torch.float32, got {out_dtype}")
        _, per, size, _ = gguf.TYPES[ggml_type]
        self._chk(blocks, torch.uint8, "dequant_gguf: blocks")
        if blocks.numel() == 0 or blocks.numel() % size:
            raise ValueError(f"dequant_gguf: blocks must hold whole {gguf.type_name(ggml_type)} blocks of {size} bytes, got "
                             f"{blocks.numel()} bytes")
        n = blocks.numel() // size
        out = self._out("dequant_gguf", out, (n, per), out_dtype)
        if blocks.data_ptr() % 32:
            blocks = blocks.clone()
        kind = 1 if out_dtype == torch.float32 else 0                        # SVR_STORE_FP32 / SVR_STORE_BF16
        self._launch("svr_dequant_gguf", _ptr(blocks), int(ggml_type), n, _ptr(out), kind, out.numel() * out.element_size())
        return out

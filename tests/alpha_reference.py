"""The alpha fixture: tests/golden/recorded_alpha.pt and the recipe that records it from the reference's own code.

The reference's src/core/alpha_upscaling.py imports cv2, which is not installed where this suite runs, so its four functions
(detect_edges_batch, guided_filter_pytorch, _apply_guided_filter, edge_guided_alpha_upscale) are compiled from the unmodified text
(oracle.reference_loader._extract) into a namespace that provides torch / F / np, a move-and-cast manage_tensor, the fp32 cast of
ensure_float32_precision and ``Cv2Standin`` below: cvtColor(RGB2GRAY) and Sobel(ksize=3, CV_64F) written from OpenCV's published
definitions (8-bit RGB2GRAY = (4899 R + 9617 G + 1868 B + 8192) >> 14; Sobel = [1 2 1] x [-1 0 1] with BORDER_REFLECT_101).
LIMITATION: the fixture therefore pins the reference's code PLUS that stand-in, not OpenCV's binaries.

Per case the fixture holds the inputs (rgb, alpha_lo), the edge bytes, the bicubic base, the reference's fp32 output ``ref32``, the
same functions run in double precision (``ref64``, stored as the fp32 difference ref64 - ref32 to keep the file small: 1e-13 of
rounding), E = max |ref32 - ref64| and a ``fragile`` mask: pixels whose output moves by more than 1e-3 when the guided filter's
result is shifted by +-1e-4 (a threshold flip moves a pixel by tenths; the smooth part by at most 3e-4, the sigmoid's slope being 3).
The recorder asserts fragile <= 0.1 % of a case, so a test cannot hide a failure behind the mask.

Recording happens only where the reference CHECKOUT is present (reference_loader.kind() == "source", SVR_RECORD_REFERENCE=1);
everywhere else -- the byte-compiled oracle/_ref has no definitions of this module -- the file is loaded as it is.
"""
import os
import typing

import numpy as np
import torch
import torch.nn.functional as F

from conftest import GOLDEN, recorded

FIXTURE = os.path.join(GOLDEN, "recorded_alpha.pt")
FUNCTIONS = ["detect_edges_batch", "guided_filter_pytorch", "_apply_guided_filter", "edge_guided_alpha_upscale"]

# name -> (T, (H, W) upscaled, (h, w) input, rgb range, overshoot below -1)
CASES = {
    "tiny_5x7": (1, (5, 7), (3, 4), "signed", False),               # smaller than either filter window
    "tile_edge_33x37": (3, (33, 37), (9, 11), "signed", False),     # one pixel past a 32-tile; very different edge maxima
    "ragged_70x118": (2, (70, 118), (24, 40), "signed", False),     # ragged multi-tile
    "unit_range_20x24": (2, (20, 24), (6, 8), "unit", False),       # rgb already in [0, 1]: never normalised
    "overshoot_20x24": (2, (20, 24), (6, 8), "signed", True),       # a few pixels below -1: the edge image is normalised twice
}
MATTES = ("binary", "soft")


class Cv2Standin:
    COLOR_RGB2GRAY, CV_64F = 7, 6

    @staticmethod
    def cvtColor(frame, code):
        assert code == Cv2Standin.COLOR_RGB2GRAY and frame.dtype == np.uint8
        f = frame.astype(np.int64)
        return ((4899 * f[..., 0] + 9617 * f[..., 1] + 1868 * f[..., 2] + 8192) >> 14).astype(np.uint8)

    @staticmethod
    def Sobel(src, ddepth, dx, dy, ksize=3):
        assert ddepth == Cv2Standin.CV_64F and ksize == 3 and (dx, dy) in ((1, 0), (0, 1))
        H, W = src.shape
        p = np.pad(src.astype(np.float64), 1, mode="reflect")          # numpy's "reflect" is BORDER_REFLECT_101
        smooth, deriv = (1.0, 2.0, 1.0), (-1.0, 0.0, 1.0)
        ky, kx = (deriv if dy else smooth), (deriv if dx else smooth)
        out = np.zeros((H, W), np.float64)
        for i in range(3):
            for j in range(3):
                out += ky[i] * kx[j] * p[i:i + H, j:j + W]
        return out


def scene(name):
    """-> (rgb [T, H, W, 3] fp32, {"binary": alpha_lo, "soft": alpha_lo} [T, h, w]): a disc moving over a smooth texture."""
    T, (H, W), (h, w), rng, overshoot = CASES[name]
    contrast = (1.0, 0.12, 0.5)                                          # per frame: very different Sobel maxima

    def disc(hh, ww, t):
        y = (torch.arange(hh, dtype=torch.float64) + 0.5) / hh
        x = (torch.arange(ww, dtype=torch.float64) + 0.5) / ww
        cy, cx = 0.45 + 0.07 * t, 0.4 + 0.11 * t
        return ((y[:, None] - cy) ** 2 + ((x[None, :] - cx) * ww / hh) ** 2).sqrt()     # distance in units of the height

    frames, binary, soft = [], [], []
    for t in range(T):
        y = torch.arange(H, dtype=torch.float64)[:, None]
        x = torch.arange(W, dtype=torch.float64)[None, :]
        d = disc(H, W, t)
        inside = torch.sigmoid((0.3 - d) * 25.0)
        chans = []
        for c in range(3):
            tex = 0.5 + 0.22 * torch.sin(0.37 * x + 0.5 * c + 0.3 * t) * torch.cos(0.23 * y - 0.4 * c)
            fg = 0.75 - 0.2 * c + 0.1 * torch.sin(0.11 * (x + y))
            chans.append(0.5 + contrast[t % 3] * ((1 - inside) * tex + inside * fg - 0.5))
        frames.append(torch.stack(chans, dim=-1))
        dl = disc(h, w, t)
        binary.append((dl < 0.3).double())
        soft.append(torch.exp(-(dl / 0.35) ** 2))
    rgb = torch.stack(frames)
    if rng == "signed":
        rgb = rgb * 2 - 1
    if overshoot:
        rgb[0, 1, 2, :] = torch.tensor([-1.06, -1.02, -1.0], dtype=torch.float64)
        rgb[1, H - 2, W - 3, 1] = -1.11
    return rgb.float(), {"binary": torch.stack(binary).float(), "soft": torch.stack(soft).float()}


def reference_functions(double=False, q_shift=0.0):
    """The reference's four functions in a namespace of fp32 (or fp64) casts.  ``q_shift`` is added to guided_filter_pytorch's
    result (the fragile mask).  In the fp64 namespace the edge detector stays the fp32 one: its bytes are part of the inputs."""
    from oracle import reference_loader as rl

    def manage_tensor(tensor, target_device=None, tensor_name=None, dtype=None, **kw):
        return tensor.to(device=target_device if target_device is not None else tensor.device, dtype=dtype or tensor.dtype)

    cast = (lambda t, force_float32=True: (t.double(), t.dtype)) if double else (lambda t, force_float32=True: (t.float(), t.dtype))
    ns = {"torch": torch, "F": F, "np": np, "cv2": Cv2Standin, "Optional": typing.Optional, "Any": typing.Any, "List": typing.List,
          "ensure_float32_precision": cast, "manage_tensor": manage_tensor}
    rl._extract("src/core/alpha_upscaling.py", FUNCTIONS, ns)
    if double:
        edges32 = reference_functions()["detect_edges_batch"]
        ns["detect_edges_batch"] = lambda images, method="sobel", debug=None: edges32(images=images.float(), method=method).double()
    if q_shift:
        plain = ns["guided_filter_pytorch"]
        ns["guided_filter_pytorch"] = lambda guide, src, radius=8, eps=0.01: plain(guide, src, radius, eps) + q_shift
    return ns


def _nchw(rgb_thwc):
    return rgb_thwc.permute(0, 3, 1, 2).contiguous()


def run_reference(rgb_thwc, alpha_lo, double=False, q_shift=0.0):
    """edge_guided_alpha_upscale(method='guided') on [T, H, W, 3] / [T, h, w] -> [T, H, W]."""
    ns = reference_functions(double, q_shift)
    dt = torch.float64 if double else torch.float32
    out = ns["edge_guided_alpha_upscale"](input_alpha=alpha_lo.to(dt).unsqueeze(1), input_rgb=torch.zeros(1, dtype=dt),
                                          upscaled_rgb=_nchw(rgb_thwc).to(dt), method="guided")
    return out.squeeze(1)


def record_case(name):
    rgb, mattes = scene(name)
    T, (H, W), _, _, _ = CASES[name]
    ns = reference_functions()
    x = _nchw(rgb)
    if x.min() < 0:                                                       # what edge_guided_alpha_upscale hands the detector
        x = (x + 1) / 2
    edge = (ns["detect_edges_batch"](images=x, method="sobel").squeeze(1) * 255.0).round().to(torch.uint8)
    case = {"rgb": rgb, "edge": edge}
    for kind in MATTES:
        a = mattes[kind]
        ref32 = run_reference(rgb, a)
        ref64 = run_reference(rgb, a, double=True)
        moved = torch.zeros_like(ref32, dtype=torch.bool)
        for s in (1e-4, -1e-4):
            moved |= (run_reference(rgb, a, q_shift=s) - ref32).abs() > 1e-3
        assert float(moved.float().mean()) <= 1e-3, (name, kind, int(moved.sum()))
        delta = ref64 - ref32.double()
        E = float(delta.abs()[~moved].max())
        assert E < 1e-4, (name, kind, E)                                   # two realisations of the same arithmetic, fp32 vs fp64
        base = F.interpolate(a.unsqueeze(1), size=(H, W), mode="bicubic", align_corners=False, antialias=True).clamp(0, 1).squeeze(1)
        case[kind] = {"alpha_lo": a, "base": base, "ref32": ref32, "ref64_minus_ref32": delta.float(), "E": E, "fragile": moved}
    return case


def load_cases():
    """name -> case dict with ``ref64`` rebuilt in fp64: run live (and recorded under SVR_RECORD_REFERENCE=1) where the reference
    checkout is present, else read from the fixture."""
    from oracle import reference_loader as rl
    if rl.available() and rl.kind() == "source":
        cases = {name: recorded("alpha", name, lambda name=name: record_case(name)) for name in CASES}
    else:
        assert os.path.exists(FIXTURE), f"{FIXTURE} is missing: record it where the reference checkout is available"
        cases = torch.load(FIXTURE, weights_only=True)
        assert set(cases) >= set(CASES), sorted(set(CASES) - set(cases))
    out = {}
    for name in CASES:
        c = dict(cases[name])
        for kind in MATTES:
            m = dict(c[kind])
            m["ref64"] = m["ref32"].double() + m["ref64_minus_ref32"].double()
            c[kind] = m
        out[name] = c
    return out


def bound(case_kind):
    """4 x E: the code under test is a second fp32 realisation of the arithmetic ref32 realises, so up to 2 E from ref64's side of
    ref32, with 2 x headroom."""
    return 4.0 * case_kind["E"]

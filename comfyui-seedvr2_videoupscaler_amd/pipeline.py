"""The four generation phases around the runner, kept entirely on the device.

Mirrors ``encode_all_batches -> upscale_all_batches -> decode_all_batches -> postprocess_all_batches``
(reference: src/core/generation_phases.py:171-540, 542-805, 807-1058, 1060-1400) for RGB input:

  * batching with ``temporal_overlap`` (step = batch_size - overlap; a trailing batch that holds only overlap
    frames is dropped, :349-357), ``uniform_batch_size`` padding with reversed frames (:71-105), the 4n+1
    rule (:398-404), the input transform (generation_utils.py:72-84) and optional input noise (:413-428);
  * per batch: seed reset (:663), ``noise = randn_like(latent)``, ``aug_noise = noise*0.1 + randn*0.05``,
    optional latent noise through the schedule (:680-697), ``get_condition(task="sr")``, one DiT step;
  * decode, trim to the original batch length and to ``true_target_dims`` (:953-968), Hann blend of the
    overlapping frames (:973-1000), write into the preallocated output;
  * for RGBA input, the alpha of every written span from the decoded frames in their [-1, 1] state BEFORE colour correction
    (:1143-1217 -> alpha.py), phases 1-3 and the colour fix seeing the RGB channels only;
  * colour correction against the re-transformed input (:1255-1320), ``[-1, 1] -> [0, 1]`` (:1348).

Differences by design (MI355X-first, results unchanged): nothing leaves the GPU between phases (the reference
round-trips every latent through host RAM by default) and with 288 GB the default is to keep the
whole output clip in HBM.  Temporal batches are independent units, which is what ``dist.py`` shards over ranks.
"""
from dataclasses import dataclass
import inspect
from typing import Callable, List, Optional, Sequence, Tuple

import torch

from . import active, alpha as alpha_mod, colorfix, shots, transforms


@dataclass
class BatchPlan:
    start: int          # first input frame of the batch
    end: int            # one past the last input frame
    uniform_pad: int    # reversed frames appended so that every batch has batch_size frames


def plan_batches(total_frames: int, batch_size: int, temporal_overlap: int = 0,
                 uniform_batch_size: bool = False) -> Tuple[List[BatchPlan], int]:
    """Batch boundaries of encode_all_batches (generation_phases.py:300-360).  Returns (plans, overlap actually used)."""
    if total_frames <= 0:
        raise ValueError("No frames to process")
    step = batch_size - temporal_overlap if temporal_overlap > 0 else batch_size
    if step <= 0:
        step, temporal_overlap = batch_size, 0
    plans = []
    for idx in range(0, total_frames, step):
        end = min(idx + batch_size, total_frames)
        if idx > 0 and end - idx <= temporal_overlap:
            break
        cur = end - idx
        plans.append(BatchPlan(idx, end, batch_size - cur if (uniform_batch_size and cur < batch_size) else 0))
    return plans, temporal_overlap


def prepare_batch(images_thwc: torch.Tensor, plan: BatchPlan, resolution: int, max_resolution: int = 0,
                  dtype: Optional[torch.dtype] = None, size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """frames [start, end) -> uniform padding -> 4n+1 padding -> input transform: [3, T', H', W'] in [-1, 1].
    ``dtype``: cast the frames BEFORE padding / resizing, as phase 1 of the reference does (the batch goes to the
    compute dtype at generation_phases.py:377-385, so its resize result, clamp, pad and normalise are rounded to bf16
    step by step); phase 4 re-transforms the input in its own dtype (generation_phases.py:127-168) -> ``None``.
    ``size``: transforms.video_transform's (``upscale(target_size=...)``)."""
    video = images_thwc[plan.start:plan.end]
    if dtype is not None:
        video = video.to(dtype)
    if plan.uniform_pad > 0:
        video = transforms.pad_video_temporal(video, count=plan.uniform_pad, temporal_dim=0, prepend=False)
    video = video.permute(0, 3, 1, 2)                                    # T C H W
    if video.size(0) % 4 != 1:
        video = transforms.pad_video_temporal(video, temporal_dim=0, prepend=False)
    return transforms.video_transform(video[:, :3], resolution, max_resolution, size=size)


def transformed_shape(images_thwc: torch.Tensor, plan: BatchPlan, resolution: int, max_resolution: int = 0,
                      size: Optional[Tuple[int, int]] = None) -> Tuple[int, ...]:
    """Shape of prepare_batch()'s result without computing it: [3, T', H', W']."""
    t = plan.end - plan.start + plan.uniform_pad
    if t % 4 != 1:
        t = ((t - 1) // 4 + 1) * 4 + 1
    if size is not None:
        h, w = transforms.check_size(size)
    else:
        h, w = transforms.resized_output_size(images_thwc.shape[1], images_thwc.shape[2], resolution)
        if max_resolution > 0 and max(h, w) > max_resolution:
            scale = max_resolution / max(h, w)
            h, w = round(h * scale), round(w * scale)
    return (3, t, (h + 15) // 16 * 16, (w + 15) // 16 * 16)


def _takes_keep_frames(runner) -> bool:
    """Only this repo's runner knows ``vae_decode(..., keep_frames=)``; any object with the reference's three calls still works."""
    try:
        return "keep_frames" in inspect.signature(runner.vae_decode).parameters
    except (TypeError, ValueError):
        return False


@torch.no_grad()
def upscale(images_thwc: torch.Tensor, runner, text_pos: torch.Tensor, *, resolution: int = 1080,
            max_resolution: int = 0, batch_size: int = 5, uniform_batch_size: bool = False,
            temporal_overlap: int = 0, prepend_frames: int = 0, color_correction: str = "lab",
            input_noise_scale: float = 0.0, latent_noise_scale: float = 0.0, seed: int = 42,
            batch_filter: Optional[Callable[[int], bool]] = None,
            progress: Optional[Callable[[str, int, int], None]] = None,
            noise_provider: Optional[Callable[[torch.Tensor], Tuple[torch.Tensor, torch.Tensor]]] = None,
            exchange_heads: Optional[Callable[[dict, list, tuple, torch.dtype], dict]] = None,
            return_spans: bool = False, skip_trimmed_frames: bool = True, output_dtype: Optional[torch.dtype] = torch.float32,
            target_size: Optional[Tuple[int, int]] = None, area=None):
    """images [T, H, W, 3] in [0, 1] (any float dtype, on the runner's device) -> upscaled [T, H', W', 3] in [0, 1].
    [T, H, W, 4] (RGBA) -> [T, H', W', 4]: the RGB channels exactly as for the three-channel clip, the fourth the edge-guided
    upscaled alpha (alpha.py) of each owned span, computed from the span's decoded frames and the input alpha of the same clip
    frames; frames of spans this rank does not own stay zero in all four channels.

    ``batch_filter(i)`` restricts phases 1-3 to the temporal batches a rank owns (data parallelism over
    batches); frames of skipped batches are left at zero for the caller's all-gather/sum.
    ``output_dtype`` (default fp32 = ComfyUI's IMAGE dtype; +0.7 dB at production width): what the decoded frames
    are held in from the decoder's output on -- the clip buffer ``final``, the overlap heads exchanged between ranks and the
    gathered clip of dist.upscale_sharded.  Memory / xGMI cost: 99.5 MB per 4K frame in fp32 against 49.8 MB in bf16 (a 128-frame
    4K clip: 12.7 GB per rank, 1.6 GB per rank on the wire at 8 ranks -- sized for 288 GB of HBM); ``output_dtype=None`` keeps the
    engines' activation dtype (bf16) as the reference's phase code does, for clips where that matters more than the 0.7 dB.

    ``target_size=(h, w)`` (None: everything above, unchanged): two even positive integers.  The input transform resizes straight
    to (h, w) with one antialiased bicubic -- no side rule, no ``max_resolution`` step; ``resolution`` and ``max_resolution`` are
    unused --, clamp, pad-to-16 and normalise follow as ever, and the decoded frames are trimmed to (h, w).  Refused together with
    ``batch_filter``, ``exchange_heads`` and ``return_spans``.

    ``area`` (None: everything above, unchanged): the active picture area of a letterboxed or pillarboxed clip (active.py, DESIGN.md
    7.3g), an explicit (y0, y1, x0, x1) in input pixels -- 0 <= y0 < y1 <= H, at least 16 rows, the columns likewise -- or an
    active.Rule, which is given the profile of the frames this call receives (before ``prepend_frames``, which only mirrors them;
    active.profile through the runner's backend: one launch and ONE read-back of H + W counts, the feature's only host
    synchronisation).  An area that is the whole frame is this call without ``area``: the same bits.  Otherwise, with
    (TH, TW) = transforms.true_target_dims and rect = active.out_rect(area, H, W, TH, TW):
        canvas = clamp(transforms.side_resize(frames as [T, C, H, W] fp32, resolution, max_resolution), 0, 1)[..., :TH, :TW]
                 as [T, TH, TW, C] in the output dtype, every channel, alpha too
        canvas[:, oy0:oy1, ox0:ox1] = upscale(frames[:, y0:y1, x0:x1].contiguous(), ..., target_size=(oy1 - oy0, ox1 - ox0))
    with every other keyword unchanged: outside the picture the result is the plain resize of what the source had there, inside
    it the model's output for the picture alone.  Memory: one extra clip-sized buffer, the canvas, next to the crop's output
    while it is copied in.  Refused together with ``batch_filter``, ``exchange_heads``, ``return_spans`` and ``target_size``.
    """
    if images_thwc.dim() != 4 or images_thwc.shape[-1] not in (3, 4):
        raise ValueError(f"images must be [T, H, W, 3] (RGB) or [T, H, W, 4] (RGBA), got {tuple(images_thwc.shape)}")
    if area is not None:
        for name, given in (("batch_filter", batch_filter), ("exchange_heads", exchange_heads), ("return_spans", return_spans),
                            ("target_size", target_size)):
            if given:
                raise ValueError(f"upscale: {name} is not served with area (the picture is a clip of its own, on one GPU)")
        kw = dict(resolution=resolution, max_resolution=max_resolution, batch_size=batch_size, uniform_batch_size=uniform_batch_size,
                  temporal_overlap=temporal_overlap, prepend_frames=prepend_frames, color_correction=color_correction,
                  input_noise_scale=input_noise_scale, latent_noise_scale=latent_noise_scale, seed=seed, progress=progress,
                  noise_provider=noise_provider, skip_trimmed_frames=skip_trimmed_frames, output_dtype=output_dtype)
        return _upscale_area(images_thwc, runner, text_pos, area, kw)
    if target_size is not None:
        target_size = transforms.check_size(target_size)
        for name, given in (("batch_filter", batch_filter), ("exchange_heads", exchange_heads), ("return_spans", return_spans)):
            if given:
                raise ValueError(f"upscale: {name} is not served with target_size")
    # compute / storage dtype of the phases = the engines' activation dtype (bf16 on the HIP path, as the reference's
    # compute_dtype; fp32 when the CPU tests drive the engines with the fp32 torch double of the C ABI)
    dev, dt = runner.dit.device, getattr(getattr(runner.dit, "ops", None), "act_dtype", torch.bfloat16)
    # what the decoded frames are held in from the decoder's output on (trims, overlap blend, colour fix, [-1, 1] -> [0, 1]) and
    # returned in.  Default fp32 = ComfyUI's IMAGE dtype (video_upscaler.py:241): a bf16 [0, 1] frame has a step of 2^-8 above 0.5,
    # i.e. 1.1e-3 rms of rounding per stage -- 1.3e-6 of the 1e-5 MSE that 50 dB allows (tools/error_budget.py);
    # None: the engines' activation dtype (rounds 2-3; the reference keeps final_video in its compute dtype)
    odt = output_dtype if output_dtype is not None else dt
    images = images_thwc.to(device=dev)
    if prepend_frames > 0:
        images = transforms.pad_video_temporal(images, count=prepend_frames, temporal_dim=0, prepend=True)
    alpha_in = None
    if images.shape[-1] == 4:
        # (the RGB copy has the strides of a three-channel clip, so phases 1-3 and the colour fix compute the same bits)
        alpha_in, images = images[..., 3], images[..., :3].contiguous()
    total = images.shape[0]
    true_h, true_w = (transforms.true_target_dims(images.shape[1], images.shape[2], resolution, max_resolution)
                      if target_size is None else target_size)
    plans, overlap = plan_batches(total, batch_size, temporal_overlap, uniform_batch_size)
    mine = [i for i in range(len(plans)) if batch_filter is None or batch_filter(i)]

    # ---- phase 1: encode.  The input noise comes from ONE generator stream seeded with seed + 1e6 before the first
    # batch (set_seed(seed_vae), generation_phases.py:327-330) and consumed batch after batch; a rank that skips batches
    # (batch_filter) draws and discards their noise, so every batch sees the noise of the single-rank run.
    latents = {}
    if input_noise_scale > 0:
        torch.manual_seed(seed + 1_000_000)
        if dev.type == "cuda":
            torch.cuda.manual_seed(seed + 1_000_000)
    owned = set(mine)
    done = 0
    for i, plan in enumerate(plans):
        if i not in owned:
            if input_noise_scale > 0 and i < max(mine, default=-1):
                c, t, h, w = transformed_shape(images, plan, resolution, max_resolution, size=target_size)
                # same shape AND strides as prepare_batch's result (a [T, C, H, W] buffer viewed c t h w): the CPU generator
                # consumes its stream differently for contiguous and strided outputs
                torch.randn_like(torch.empty((t, c, h, w), dtype=dt, device=dev).permute(1, 0, 2, 3))
            continue
        x = prepare_batch(images, plan, resolution, max_resolution, dtype=dt, size=target_size)
        if input_noise_scale > 0:
            noise = torch.randn_like(x) * 0.05
            blend = input_noise_scale * 0.5
            x = x * (1 - blend) + (x + noise) * blend
        latents[i] = runner.vae_encode([x])[0]
        done += 1
        if progress:
            progress("encode", done, len(mine))

    # ---- phase 2: one-step DiT
    upscaled = {}
    for n, i in enumerate(mine):
        latent = latents.pop(i).to(dt)
        torch.manual_seed(seed)                        # identical RNG state for every batch (generation_phases.py:663)
        if dev.type == "cuda":
            torch.cuda.manual_seed(seed)
        if noise_provider is None:
            base_noise = torch.randn_like(latent)
            extra = torch.randn_like(base_noise)
        else:
            base_noise, extra = (t.to(device=dev, dtype=dt) for t in noise_provider(latent))
        aug_noise = base_noise * 0.1 + extra * 0.05
        blur = latent
        if latent_noise_scale != 0.0:
            t = torch.tensor([1000.0], device=dev, dtype=dt) * latent_noise_scale
            shape = torch.tensor(latent.shape[1:], device=dev)[None]
            blur = runner.schedule.forward(latent, aug_noise, runner.timestep_transform(t, shape))
        cond = runner.get_condition(base_noise, task="sr", latent_blur=blur)
        upscaled[i] = runner.inference([base_noise], [cond], [text_pos], [text_pos])[0]
        if progress:
            progress("upscale", n + 1, len(mine))

    # ---- phase 3: decode, trim, blend into the output clip ([-1, 1] until phase 4)
    final = torch.zeros(total, true_h, true_w, 3, dtype=odt, device=dev)
    spans, heads, starts = {}, {}, {}
    write = 0
    for i, plan in enumerate(plans):
        starts[i] = write
        ori = plan.end - plan.start
        n_new = ori if (i == 0 or overlap == 0) else max(ori - overlap, 0)
        if i in upscaled:
            # (skip_trimmed_frames: the decoder is causal in time, so our runner leaves out the padding frames that are trimmed
            # two lines down -- same result, bit for bit on the HIP path (tests/test_gpu_parity.py::test_vae_decode_keep_frames_bit_exact))
            sample = (runner.vae_decode([upscaled.pop(i)], keep_frames=[ori])[0]
                      if skip_trimmed_frames and _takes_keep_frames(runner) else runner.vae_decode([upscaled.pop(i)])[0])
            if sample.dim() == 3:
                sample = sample.unsqueeze(1)
            sample = sample.permute(1, 2, 3, 0)[:ori, :true_h, :true_w].to(odt)           # T H W C, padding trimmed
            if i > 0 and 0 < overlap < sample.shape[0] and write >= overlap:
                if (i - 1) in spans:                                                      # both sides are on this rank
                    final[write - overlap:write] = transforms.blend_overlapping_frames(
                        final[write - overlap:write], sample[:overlap], overlap)
                else:
                    heads[i] = sample[:overlap].contiguous()                              # blended by the previous batch's owner
                sample = sample[overlap:]
            final[write:write + sample.shape[0]] = sample
            spans[i] = (write, write + sample.shape[0])
            if progress:
                progress("decode", len(spans), len(mine))
        write += n_new

    if exchange_heads is not None and overlap > 0:
        # batch boundaries that carry an overlap blend -- a function of the plans alone, so every rank derives the same list
        # and the point-to-point exchange posts matching sends and receives
        boundaries = [i for i, plan in enumerate(plans) if i > 0 and 0 < overlap < plan.end - plan.start and starts[i] >= overlap]
        for i, head in exchange_heads(heads, boundaries, (overlap, true_h, true_w, 3), odt).items():    # (heads travel in the frames' dtype)
            if (i - 1) in spans and i not in spans:
                w = starts[i]
                final[w - overlap:w] = transforms.blend_overlapping_frames(final[w - overlap:w], head.to(final), overlap)

    # ---- phase 4: alpha from the frames as decoded (before colour correction, the reference's order), then colour correction
    # against the re-transformed input, [-1, 1] -> [0, 1].  A span's frames in ``final`` ARE clip frames w0..w1 (overlap heads are
    # trimmed before the write), so its alpha is guided by the input alpha of exactly those frames.
    alpha_out = torch.zeros(total, true_h, true_w, dtype=odt, device=dev) if alpha_in is not None else None
    for i, (w0, w1) in spans.items():
        if w1 <= w0:
            continue
        if alpha_in is not None:
            alpha_out[w0:w1] = alpha_mod.upscale_alpha(final[w0:w1], alpha_in[w0:w1], getattr(runner.dit, "ops", None)).to(odt)
        sample = final[w0:w1].permute(0, 3, 1, 2)
        if color_correction != "none":
            ref = prepare_batch(images, plans[i], resolution, max_resolution, size=target_size).to(odt).permute(1, 0, 2, 3)   # T C H W
            if i > 0 and overlap > 0:
                ref = ref[overlap:]
            ref = ref[:sample.shape[0], :, :true_h, :true_w]
            if color_correction not in colorfix.METHODS:
                raise ValueError(f"Unknown color correction method: {color_correction}")
            sample = colorfix.correct(sample, ref, color_correction, ops=getattr(runner.dit, "ops", None))
        final[w0:w1] = sample.permute(0, 2, 3, 1).clamp(-1, 1).mul(0.5).add(0.5).to(odt)
    if alpha_out is not None:
        final = torch.cat([final, alpha_out.unsqueeze(-1)], dim=-1)
    if prepend_frames > 0:
        final = final[prepend_frames:]
        spans = {i: (max(a - prepend_frames, 0), max(b - prepend_frames, 0)) for i, (a, b) in spans.items()}
    return (final, spans) if return_spans else final


def _upscale_area(images_thwc: torch.Tensor, runner, text_pos: torch.Tensor, area, kw: dict) -> torch.Tensor:
    """``upscale(area=...)``: the statement in its docstring, line by line."""
    T, H, W, _ = images_thwc.shape
    if T == 0:
        raise ValueError("No frames to process")
    dev = runner.dit.device
    if isinstance(area, active.Rule):
        frames = images_thwc if images_thwc.dtype in (torch.float32, torch.bfloat16) else images_thwc.float()
        counts = active.profile(frames.to(dev).contiguous(), area.dark, getattr(runner.dit, "ops", None)).tolist()   # the one read-back
        area = area.area(counts, T, H, W)
    else:
        ok = isinstance(area, (tuple, list)) and len(area) == 4 and all(isinstance(v, int) and not isinstance(v, bool) for v in area)
        if not ok:
            raise ValueError(f"area must be an active.Rule or (y0, y1, x0, x1) in integers, got {area!r}")
        y0, y1, x0, x1 = area
        if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W) or y1 - y0 < active.MIN_SIDE or x1 - x0 < active.MIN_SIDE:
            raise ValueError(f"area must satisfy 0 <= y0 < y1 <= H = {H}, 0 <= x0 < x1 <= W = {W} with at least "
                             f"{active.MIN_SIDE} rows and columns, got {tuple(area)}")
    y0, y1, x0, x1 = area
    if (y0, y1, x0, x1) == (0, H, 0, W):
        return upscale(images_thwc, runner, text_pos, **kw)
    true_h, true_w = transforms.true_target_dims(H, W, kw["resolution"], kw["max_resolution"])
    oy0, oy1, ox0, ox1 = active.out_rect((y0, y1, x0, x1), H, W, true_h, true_w)
    odt = kw["output_dtype"] if kw["output_dtype"] is not None else getattr(getattr(runner.dit, "ops", None), "act_dtype", torch.bfloat16)
    images = images_thwc.to(device=dev)
    canvas = transforms.side_resize(images.permute(0, 3, 1, 2).float(), kw["resolution"], kw["max_resolution"])
    canvas = canvas.clamp(0.0, 1.0)[..., :true_h, :true_w].permute(0, 2, 3, 1).to(odt).contiguous()
    out = upscale(images[:, y0:y1, x0:x1].contiguous(), runner, text_pos, target_size=(oy1 - oy0, ox1 - ox0), **kw)
    canvas[:, oy0:oy1, ox0:ox1] = out
    return canvas


def _signatures(frames: torch.Tensor, runner) -> torch.Tensor:
    """shots.signatures of clip frames on the runner's device, through the runner's backend (dense, fp32 unless bf16)."""
    if frames.dtype not in (torch.float32, torch.bfloat16):
        frames = frames.float()
    return shots.signatures(frames.to(runner.dit.device).contiguous(), getattr(runner.dit, "ops", None))


def _refuse_for_shots(who: str, upscale_kwargs: dict):
    for name in ("batch_filter", "exchange_heads", "return_spans"):
        if upscale_kwargs.get(name):
            raise ValueError(f"{who}: {name} is not served with cuts (a shot is a clip of its own; sharding one over ranks is out of scope)")


@torch.no_grad()
def upscale_shots(images_thwc: torch.Tensor, runner, text_pos: torch.Tensor, *, cuts, **upscale_kwargs):
    """``upscale`` with no batch across a cut: every shot is a clip of its own.  ``cuts``: a sorted list of the frame indices that
    start a shot (shots.split's rule), or a shots.Detector, which is fed the signatures of the clip (shots.signatures through the
    runner's backend: one launch and one read-back of T distances).  The result is, bit for bit, the concatenation of
    ``upscale(images[a:b], ...same keyword arguments...)`` over the shots [a, b): ``prepend_frames``, ``uniform_batch_size``, the
    noise seeds and the overlap blend all apply per shot.  ``batch_filter``, ``exchange_heads`` and ``return_spans`` are refused.
    ``area=`` is one of the forwarded keyword arguments, so it is served per shot without a line here: a Rule sees each shot's own
    frames (aspect ratios change at cuts), a letterboxed shot is cropped and its neighbour is not."""
    _refuse_for_shots("upscale_shots", upscale_kwargs)
    if images_thwc.dim() != 4 or images_thwc.shape[-1] not in (3, 4) or images_thwc.shape[0] == 0:
        raise ValueError(f"images must be [T >= 1, H, W, 3] (RGB) or [T >= 1, H, W, 4] (RGBA), got {tuple(images_thwc.shape)}")
    if isinstance(cuts, shots.Detector):
        first = cuts.count
        cuts = [c - first for c in cuts.feed(_signatures(images_thwc, runner))]
    spans = shots.split(images_thwc.shape[0], cuts)
    if len(spans) == 1:
        return upscale(images_thwc, runner, text_pos, **upscale_kwargs)
    return torch.cat([upscale(images_thwc[a:b], runner, text_pos, **upscale_kwargs) for a, b in spans], dim=0)


def _upscale_stream_shots(chunks, runner, text_pos, cuts, temporal_overlap, prepend_frames, upscale_kwargs):
    """upscale_stream with ``cuts``: each chunk in pieces that end at its cuts."""
    _refuse_for_shots("upscale_stream", upscale_kwargs)
    detector = cuts if isinstance(cuts, shots.Detector) else None
    if detector is None:
        cuts = [int(c) for c in cuts]
        if any(c < 0 for c in cuts) or any(b <= a for a, b in zip(cuts, cuts[1:])):
            raise ValueError(f"cuts must be strictly increasing frame indices, got {cuts}")
    tail, base, shot_start = None, 0, 0                  # base: the clip index of the chunk's first frame; shot_start: of its shot's
    for k, chunk in enumerate(chunks):
        if chunk.dim() != 4 or chunk.shape[0] == 0:
            raise ValueError(f"chunk {k} must be [t, H, W, 3 | 4] with t >= 1, got {tuple(chunk.shape)}")
        t = chunk.shape[0]
        if detector is not None:
            first = detector.count
            local = [c - first for c in detector.feed(_signatures(chunk, runner))]
        else:
            local = [c - base for c in cuts if base <= c < base + t]
        starts_shot = k == 0 or (bool(local) and local[0] == 0)                # (the clip's first frame starts a shot by itself)
        outs = []
        for j, (a, b) in enumerate(shots.split(t, [c for c in local if c > 0])):
            frames, context = chunk[a:b], 0
            if j == 0 and not starts_shot and tail is not None and temporal_overlap > 0:
                context = min(temporal_overlap, tail.shape[0], base - shot_start)          # never behind the last cut; >= 1
                frames = torch.cat([tail[-context:].to(chunk.device), frames], dim=0)
            out = upscale(frames, runner, text_pos, temporal_overlap=temporal_overlap,
                          prepend_frames=prepend_frames if (j > 0 or starts_shot) else 0, **upscale_kwargs)
            outs.append(out[context:] if context > 0 else out)
            del frames, out
        if local:
            shot_start = base + local[-1]
        base += t
        tail = chunk[-temporal_overlap:].clone() if temporal_overlap > 0 else None
        del chunk
        out = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
        del outs
        yield out
        del out


def upscale_stream(chunks, runner, text_pos: torch.Tensor, *, temporal_overlap: int = 0, prepend_frames: int = 0, cuts=None,
                   **upscale_kwargs):
    """A clip too long to hold, as a stream: ``chunks`` is any iterable of [t, H, W, 3 | 4] tensors (consecutive pieces of one
    clip), the generator yields one upscaled [t, H', W', C] tensor per chunk.  The reference's ``_stream_video_chunks``
    (inference_cli.py:621-718): chunk k > 0 is upscaled with the last min(temporal_overlap, t_prev) RAW input frames of chunk k - 1
    prepended as temporal context, whose output frames are dropped; ``prepend_frames`` applies to the first chunk only; everything
    else goes to ``upscale`` unchanged (``temporal_overlap`` also as the batch overlap inside a chunk).  So the stream equals, bit
    for bit, ``upscale`` called on each (context + chunk) with the context trimmed -- and NOT the one-call result of the whole clip
    wherever a batch boundary falls differently.

    Memory: nothing of chunk k stays referenced here once chunk k + 1 is yielded except its raw input tail (``temporal_overlap``
    input frames), so device memory is bounded by one chunk whatever the clip's length -- provided the caller drops (or packs,
    frameio.pack_frames) each yielded tensor before asking for the next.

    ``cuts`` (None: everything above, unchanged): a shots.Detector, which is fed each chunk's signatures, or a sorted list of the clip
    frame indices that start a shot.  A chunk is then split into pieces at its cuts and each piece goes through ``upscale``; the
    outputs are concatenated, so the generator still yields one tensor per chunk.  The first piece of a chunk continues the previous
    chunk's shot: it gets the usual context, shortened so that it never reaches behind the last cut -- none, and ``prepend_frames``
    instead, if the chunk's first frame is itself a cut.  Every later piece starts a shot: no context, and ``prepend_frames``.  No
    batch and no context then spans a cut; a clip without cuts streams to the same bits as with ``cuts=None``.  The memory
    statement holds: besides the raw tail the generator keeps the detector's state (one signature of 4 KB and at most ``window``
    integers), and the pieces' outputs live only until they are concatenated into the chunk's.

    ``area=`` is one of the forwarded keyword arguments, so it is served per (context + chunk) call, or per piece with ``cuts``,
    without a line here: a Rule sees the frames of each call, context included, and neighbouring chunks may choose different
    areas.  The memory statement holds with one more chunk-sized buffer, ``upscale``'s canvas."""
    if cuts is not None:
        yield from _upscale_stream_shots(chunks, runner, text_pos, cuts, temporal_overlap, prepend_frames, upscale_kwargs)
        return
    tail = None
    for k, chunk in enumerate(chunks):
        if chunk.dim() != 4 or chunk.shape[0] == 0:
            raise ValueError(f"chunk {k} must be [t, H, W, 3 | 4] with t >= 1, got {tuple(chunk.shape)}")
        context = 0
        frames = chunk
        if tail is not None and temporal_overlap > 0:
            context = min(temporal_overlap, tail.shape[0])
            frames = torch.cat([tail[-context:].to(chunk.device), chunk], dim=0)
        out = upscale(frames, runner, text_pos, temporal_overlap=temporal_overlap,
                      prepend_frames=prepend_frames if k == 0 else 0, **upscale_kwargs)
        tail = chunk[-temporal_overlap:].clone() if temporal_overlap > 0 else None
        del frames, chunk
        if context > 0:
            out = out[context:]
        yield out
        del out

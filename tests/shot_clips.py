"""TEST INFRASTRUCTURE: the synthetic clips of the shot tests (tests/test_shots.py, tests/test_gpu_shots.py).

A shot is a random field panned one pixel per frame; neighbouring shots take their values from disjoint luma ranges ([0.15, 0.35]
against [0.6, 0.8]: bins 9..22 against 38..51), so a cut moves EVERY pixel to another bin -- D = 2 H W exactly -- while a pan
step only moves the pixels whose neighbour lies in another bin or cell.  Measured with shots.signatures_torch on the CPU: the pans
4-6 % of 2 H W at 32 x 48, 7-9 % at 24 x 32, 9-13 % at 19 x 23; 16 x 20 already reaches 17 % and 8 x 8 40 %, so no clip here is
smaller than 19 x 23.  ``assert_precondition`` is what every test calls before it tests anything."""
import torch

RANGES = ((0.15, 0.35), (0.6, 0.8))


def shot_clip(H, W, lengths, seed=0, channels=3):
    """[sum(lengths), H, W, channels] fp32: shot k a pan over a random field in RANGES[k % 2]; a fourth channel is random."""
    g = torch.Generator().manual_seed(seed)
    frames = []
    for k, n in enumerate(lengths):
        lo, hi = RANGES[k % 2]
        field = torch.rand(H, W + n, 3, generator=g) * (hi - lo) + lo
        frames += [field[:, i:i + W] for i in range(n)]
    clip = torch.stack(frames)
    if channels == 4:
        clip = torch.cat([clip, torch.rand(clip.shape[0], H, W, 1, generator=g)], dim=-1)
    return clip.contiguous()


def cuts_of(lengths):
    """the frame indices that start shots 1, 2, ..."""
    out, at = [], 0
    for n in lengths[:-1]:
        at += n
        out.append(at)
    return out


def assert_precondition(shots, clip, cuts):
    """every cut has D = 2 H W exactly, every other frame D <= 0.15 * 2 H W (the torch statement, on the clip's device)"""
    T, H, W, _ = clip.shape
    D = shots.distances(shots.signatures_torch(clip)).tolist()
    for t in range(1, T):
        if t in cuts:
            assert D[t - 1] == 2 * H * W, (t, D[t - 1])
        else:
            assert D[t - 1] * 100 <= 15 * 2 * H * W, (t, D[t - 1] / (2 * H * W))

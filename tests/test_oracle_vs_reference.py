"""Pin of the oracle + the package's window planner against the reference implementation: live where the reference is
available (oracle/reference_loader.py), elsewhere against its results recorded in tests/golden/recorded_*.pt (conftest.recorded)."""
import pytest
import torch

from conftest import sub, rel_err, recorded
from oracle import reference_loader as rl
from oracle import dit_oracle, vae_oracle


def _reference_boxes(name, size, num):
    fn = getattr(rl.reference_window_module(), name)
    return [(a.start, a.stop, b.start, b.stop, c.start, c.stop) for a, b, c in fn(size, num)]


@pytest.mark.parametrize("size", [(1, 16, 16), (3, 128, 128), (9, 135, 240), (5, 18, 30), (17, 135, 240),
                                  (2, 7, 11), (31, 40, 23), (4, 45, 80)])
def test_window_boxes_equal_reference(size):
    windows = sub("windows")
    for method, name in ((windows.REGULAR, "make_720Pwindows_bysize"), (windows.SHIFTED, "make_shifted_720Pwindows_bysize")):
        want = recorded("windows", f"{name}/{size}/(4, 3, 3)", lambda: _reference_boxes(name, size, (4, 3, 3)))
        assert windows.window_boxes(size, (4, 3, 3), method) == want


def test_dit_tiny_oracle_equals_reference_ragged():
    config, weights, windows = sub("config"), sub("weights"), sub("windows")
    cfg = config.DIT_TINY
    sd = weights.synth_dit_state_dict(cfg, seed=5)
    torch.manual_seed(1)
    T, H, W = 5, 36, 60
    vid = torch.randn(T, H, W, 33)
    txt = torch.randn(58, 5120)

    def live():
        ref = rl.build_reference_dit(cfg.as_dict(), {k: v.float() for k, v in sd.items()})
        with torch.no_grad():
            return ref(vid=vid.reshape(-1, 33), txt=txt, vid_shape=torch.tensor([[T, H, W]]),
                       txt_shape=torch.tensor([[58]]), timestep=torch.tensor([1000.0])).vid_sample.reshape(T, H, W, 16)

    want = recorded("dit_tiny_ragged", "out", live)
    got = dit_oracle.dit_forward(sd, cfg, vid, txt, 1000.0, windows_mod=windows)
    assert rel_err(got, want) < 2e-5


def test_vae_oracle_equals_reference_sliced():
    config, weights = sub("config"), sub("weights")
    cfg = config.VAE_V3
    sd = weights.synth_vae_state_dict(cfg, seed=9)
    torch.manual_seed(2)
    x = torch.rand(1, 3, 9, 32, 48) * 2 - 1
    z = torch.randn(1, 16, 3, 4, 6)

    def live():
        ref = rl.build_reference_vae({k: v.float() for k, v in sd.items()})   # slicing + 0.5 GiB limits on
        with torch.no_grad():
            return {"encode": ref.encode(x).latent, "decode": ref.decode(z).sample}

    want = recorded("vae_sliced", "out", live)
    with torch.no_grad():
        assert rel_err(vae_oracle.encode(x, sd, cfg), want["encode"]) < 2e-5
        assert rel_err(vae_oracle.decode(z, sd, cfg), want["decode"]) < 2e-5


def test_window_boxes_equal_reference_fuzz():
    """Randomised sweep of the window planner against the reference's window.py (both families, several window counts)."""
    import random
    windows = sub("windows")
    rnd = random.Random(1234)
    for _ in range(150):
        size = (rnd.randint(1, 40), rnd.randint(1, 140), rnd.randint(1, 250))
        num = rnd.choice([(4, 3, 3), (1, 3, 3), (2, 2, 2), (4, 4, 4)])
        for method, name in ((windows.REGULAR, "make_720Pwindows_bysize"), (windows.SHIFTED, "make_shifted_720Pwindows_bysize")):
            want = recorded("windows", f"{name}/{size}/{num}", lambda: _reference_boxes(name, size, num))
            assert windows.window_boxes(size, num, method) == want, (size, num, method)


def test_temporal_padding_and_blend_equal_reference_fuzz():
    """pad_video_temporal / blend_overlapping_frames against the reference's function text over random lengths."""
    import random
    tr = sub("transforms")
    ns = rl.reference_glue() if rl.available() else None
    rnd = random.Random(7)
    g = torch.Generator().manual_seed(7)                  # (seeded: the recorded results are those of these inputs)
    for i in range(120):
        t = rnd.randint(1, 23)
        x = torch.randn(t, 2, 3, 3, generator=g)
        count = rnd.choice([0, 0, rnd.randint(1, 30)])
        prepend = count > 0 and rnd.random() < 0.4
        got = tr.pad_video_temporal(x, count=count, temporal_dim=0, prepend=prepend)
        want = recorded("glue_fuzz", f"pad/{i}", lambda: ns["pad_video_temporal"](x.clone(), count=count, temporal_dim=0, prepend=prepend))
        assert got.shape == want.shape and torch.equal(got, want), (t, count, prepend)
    for ov in range(1, 9):
        a, b = torch.randn(ov, 4, 5, 3, generator=g), torch.randn(ov, 4, 5, 3, generator=g)
        want = recorded("glue_fuzz", f"blend/{ov}", lambda: ns["blend_overlapping_frames"](a.clone(), b.clone(), ov))
        assert torch.equal(tr.blend_overlapping_frames(a, b, ov), want)

"""TEST INFRASTRUCTURE: the ALGORITHM of the two attention kernels (csrc/svr_attn.hip, csrc/svr_attn_win.hip) in fp32 torch, with
switches that break it the way a kernel could be broken.

tests/test_local_error.py uses it as "a correct implementation" of flash attention on the score-range cases of
tests/conditioning_cases.py (attn_score_cases): the per-element bound of local_error.attn_reference must hold for the correct
algorithm on every case, and must reject each fault on the cases that can see it.  What it keeps of the kernels:

  * online softmax over ``kt``-key tiles in log2 units, p = exp2(s c - m c), c = scale log2(e);
  * the ragged last tile reads clamped duplicates of key L - 1, which only the -inf mask removes;
  * ONE rescale decision per ``qblock`` query rows: rescale when not all((mx - m) c <= defer) over the block (the window kernel's
    wave vote; ``defer=None``: every tile, the first-generation kernel) -- the whole block then takes m = max(m, mx) and multiplies
    O and l by alpha = exp2((m_old - m) c), otherwise the block keeps m and P may reach 2^defer;
  * P rounded to bf16 for the PV product, l summed from the unrounded P, fp32 accumulators, one bf16 rounding of O / l.

It is no model of lanes, fragments or LDS (tests/test_attn_win_layout.py is)."""
import torch

LOG2E = 1.4426950408889634
FAULTS = (None, "nomask", "stale_o", "stale_l")


def flash_emulation(q, k, v, scale, *, kt, qblock, defer, fault=None, decisions=None):
    """q, k, v: [L, D] (bf16 values) -> out [L, D] bf16.

    fault: "nomask" -- the clamped keys past L keep their scores; "stale_o" -- O is not multiplied by alpha when a block rescales;
    "stale_l" -- l is not.  ``decisions``: a list that receives one bool tensor [blocks] per tile (True = the block rescaled)."""
    assert fault in FAULTS, fault
    L, D = q.shape
    f32 = torch.float32
    qf, kf, vf = q.to(f32), k.to(f32), v.to(f32)
    c = torch.tensor(scale * LOG2E, dtype=f32)
    nk, nb = -(-L // kt), -(-L // qblock)
    m = torch.full((L,), float("-inf"), dtype=f32, device=q.device)
    l = torch.zeros(L, dtype=f32, device=q.device)
    O = torch.zeros(L, D, dtype=f32, device=q.device)
    for t in range(nk):
        key = torch.arange(t * kt, (t + 1) * kt, device=q.device)
        rows = key.clamp(max=L - 1)
        s = qf @ kf[rows].t()                                                      # [L, kt]
        if fault != "nomask":
            s[:, key >= L] = float("-inf")
        mx = s.amax(dim=1)
        if defer is None:
            resc = torch.ones(nb, dtype=torch.bool, device=q.device)
        else:
            ok = (mx - m) * c <= defer                                             # (first tile: m = -inf, never ok)
            ok = torch.cat([ok, ok.new_ones(nb * qblock - L)]).reshape(nb, qblock)
            resc = ~ok.all(dim=1)
        if decisions is not None:
            decisions.append(resc.clone())
        resc = resc.repeat_interleave(qblock)[:L]
        m_new = torch.where(resc, torch.maximum(m, mx), m)
        alpha = torch.exp2(m * c - m_new * c)                                      # 1 where the block kept m; 0 on the first tile
        alpha = torch.where(resc, alpha, torch.ones_like(alpha))
        m = m_new
        p = torch.exp2(s * c - (m * c)[:, None])
        l = (l if fault == "stale_l" else l * alpha) + p.sum(dim=1)
        O = (O if fault == "stale_o" else O * alpha[:, None]) + p.to(torch.bfloat16).to(f32) @ vf[rows]
    return (O / l[:, None]).to(torch.bfloat16)

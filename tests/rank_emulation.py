"""TEST INFRASTRUCTURE: a numpy restatement of the launches of csrc/svr_rank.hip as built -- the same tile, digit width, group of
tiles per workgroup, table layout, scan steps and in-tile ranking -- so that the structure of the sort (not only its result) can be
checked without a device, in the manner of tests/attn_emulation.py.

  hist     table[digit][tile] = how many keys of the tile hold the digit; tiles_p = tiles rounded up to GROUP, padding columns 0
  scan     row d -> its exclusive prefix over the tiles, SCAN_STEP entries per step with a carry; totals[d] = the row's sum
  scatter  per tile: wave w, round j, lane l holds tile position w * WAVE_KEYS + j * 64 + l (empty past the end).  A round ranks its
           64 keys by match masks: rank = per-wave digit counter + popcount(mask & lanes below); then the counter grows by
           popcount(mask).  Waves chain through their exclusive sums, digits through the exclusive scan of the tile's counts.  A key
           goes to (exclusive scan of totals)[d] + table[d][tile] + (its place among the tile's keys of digit d).

``sort(keys_u32)`` runs the four passes and returns (sorted keys, source indices)."""
import numpy as np

BITS, RADIX = 8, 256
THREADS, WAVES, KPT = 256, 4, 16
TILE = THREADS * KPT                # 4096
WAVE_KEYS = 64 * KPT                # 1024
GROUP = 16
SCAN_STEP = THREADS * 8             # 2048


def geometry(n):
    tiles = -(-n // TILE)
    groups = -(-tiles // GROUP)
    return tiles, groups, groups * GROUP


def hist(keys, shift):
    n = keys.size
    tiles, groups, tiles_p = geometry(n)
    table = np.zeros((RADIX, tiles_p), np.uint32)
    for g in range(groups):                                   # a workgroup: GROUP tiles, whole tiles past the end left out
        for tt in range(GROUP):
            base = (g * GROUP + tt) * TILE
            if base >= n:
                break
            d = (keys[base:base + TILE] >> np.uint32(shift)) & np.uint32(RADIX - 1)
            table[:, g * GROUP + tt] = np.bincount(d, minlength=RADIX)
    return table


def scan(table):
    tiles_p = table.shape[1]
    totals = np.zeros(RADIX, np.uint32)
    out = np.empty_like(table)
    for d in range(RADIX):                                    # a workgroup per row
        carry = np.uint32(0)
        for base in range(0, tiles_p, SCAN_STEP):
            step = table[d, base:base + SCAN_STEP]
            inc = np.cumsum(step, dtype=np.uint32)
            out[d, base:base + SCAN_STEP] = inc - step + carry
            carry = np.uint32(carry + (inc[-1] if inc.size else 0))
        totals[d] = carry
    return out, totals


def tile_ranks(digits):
    """digits: the nvalid <= TILE digits of one tile in tile order -> (place of each key in the tile's digit-sorted order,
    the tile's exclusive digit starts), by the kernel's rounds"""
    nvalid = digits.size
    cnt = np.zeros((WAVES, RADIX), np.int64)
    r = np.zeros(nvalid, np.int64)
    for w in range(WAVES):
        for j in range(KPT):
            p0 = w * WAVE_KEYS + j * 64
            lanes = digits[p0:min(p0 + 64, nvalid)] if p0 < nvalid else digits[:0]      # empty lanes are in no mask
            for lane, d in enumerate(lanes):
                mask = lanes == d
                r[p0 + lane] = cnt[w, d] + int(mask[:lane].sum())
            for d in np.unique(lanes):
                cnt[w, d] += int((lanes == d).sum())
    count = cnt.sum(axis=0)
    tstart = np.cumsum(count) - count
    woff = tstart[None, :] + np.cumsum(cnt, axis=0) - cnt
    place = np.empty(nvalid, np.int64)
    for p in range(nvalid):
        place[p] = woff[p // WAVE_KEYS, digits[p]] + r[p]
    return place, tstart


def scatter(keys, idx, shift, scanned, totals):
    n = keys.size
    tiles, groups, tiles_p = geometry(n)
    dbase = np.cumsum(totals, dtype=np.int64) - totals
    out_k, out_i = np.full(n, 0xDEADBEEF, np.uint32), np.full(n, 0xDEADBEEF, np.uint32)
    written = np.zeros(n, bool)
    for tile in range(tiles):
        base = tile * TILE
        k, i = keys[base:base + TILE], idx[base:base + TILE]
        d = ((k >> np.uint32(shift)) & np.uint32(RADIX - 1)).astype(np.int64)
        place, tstart = tile_ranks(d)
        sk, si = np.empty_like(k), np.empty_like(i)
        assert np.array_equal(np.sort(place), np.arange(k.size))                       # every LDS slot of the tile exactly once
        sk[place], si[place] = k, i
        sd = ((sk >> np.uint32(shift)) & np.uint32(RADIX - 1)).astype(np.int64)
        dst = dbase[sd] + scanned[sd, tile].astype(np.int64) + (np.arange(k.size) - tstart[sd])
        assert dst.min() >= 0 and dst.max() < n and not written[dst].any()
        out_k[dst], out_i[dst] = sk, si
        written[dst] = True
    assert written.all()
    return out_k, out_i


def sort(keys):
    """keys: uint32 [n] (colorfix.sort_key's values) -> (sorted keys, uint32 source indices) after four passes"""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    i = np.arange(k.size, dtype=np.uint32)
    for p in range(32 // BITS):
        shift = p * BITS
        scanned, totals = scan(hist(k, shift))
        assert int(totals.astype(np.int64).sum()) == k.size
        k, i = scatter(k, i, shift, scanned, totals)
    return k, i

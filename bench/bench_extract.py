#!/usr/bin/env python3
"""Device-tier throughput of region extraction (packed_ops.subseq_dev / extract_dev) on one MI355X, product build.  Every result
is verified in the run, before it is timed, against the same result computed with torch indexing and integer ops on the packed
words -- the route a caller had before these calls.  One JSON row per case, printed and appended to --out, every figure of a row
taken in the same run:
  subsequence rows   2^30 nt out of a 2^30 + 2^20 nt sequence, start in {0, 32*1000, 17, 2^19 + 5}, forward and reversed
    ms / min_ms / max_ms   median, fastest and slowest of --iters (>= 20) event-timed calls after a warm-up
    GBs                    bytes read + written per ns (0.5 B/nt)
    complement_ms, revcomp_ms (+ their min / max)   cnt_complement_dev and cnt_reverse_complement_dev on 2^30 nt: the same
                           traffic, the bar.  within_bar: ms <= revcomp_ms + (revcomp_max_ms - revcomp_min_ms)
  window rows        n in {2^10, 2^16, 2^20} random starts into 2^30 nt, region_len in {23, 101, 1000}, with info (half of it
                     reversed) and without
    ms, Mregions_s         as above; regions per microsecond
    torch_ms, vs_torch     the torch route for the same records; median of --torch-iters calls"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cute_nucleotides_amd as cn  # noqa: E402
from cute_nucleotides_amd import _lib, devutil, packed_ops as po  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-nt", type=int, default=30)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--torch-iters", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extract_bench.jsonl"))
a = ap.parse_args()
assert a.iters >= 20 and not _lib.is_lab_build()
STAMP = {"date": datetime.date.today().isoformat(), "build": "product"}
REVERSE = _lib.CNT_FIND_REVERSE


def timed(fn, iters):
    """(median, min, max) over `iters` calls, each between two events of its own"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def lsr(x, sh):
    """logical shift right of int64 words by a tensor of shifts 0..63"""
    sh = torch.as_tensor(sh, dtype=torch.int64, device=x.device)
    return (x >> sh) & ~((torch.full_like(sh, -1) << (63 - sh)) << 1)


def reverse_codes(x):
    x = (lsr(x, 2) & 0x3333333333333333) | ((x & 0x3333333333333333) << 2)
    x = (lsr(x, 4) & 0x0F0F0F0F0F0F0F0F) | ((x & 0x0F0F0F0F0F0F0F0F) << 4)
    return x.view(torch.uint8).view(-1, 8).flip(1).contiguous().view(torch.int64).view(x.shape)


def torch_route(bits, starts, region_len, rev, j0=0, j1=None):
    """words [j0, j1) of the records of accepted regions: gather two words per output word, funnel, reverse, mask"""
    R = (region_len + 31) // 32
    j = torch.arange(j0, R if j1 is None else j1, dtype=torch.int64, device=bits.device)[None, :]
    st = starts[:, None]
    p = torch.where(rev[:, None], st + region_len - 32 - 32 * j, st + 32 * j)
    neg = p < 0
    pp = p.clamp(min=0)
    iw, sh = pp >> 5, 2 * (pp & 31)
    lo, hi = bits[iw], bits[(iw + 1).clamp(max=bits.numel() - 1)]
    win = lsr(lo, sh) | torch.where(sh > 0, (hi << 1) << (63 - sh), torch.zeros_like(hi))
    win = torch.where(neg, bits[0] << (2 * (-p).clamp(min=0)), win)
    win = torch.where(rev[:, None], reverse_codes(win) ^ -0x5555555555555556, win)
    rem = (region_len - 32 * j).clamp(max=32)
    keep = torch.where(rem >= 32, torch.full_like(rem, -1), (torch.ones_like(rem) << (2 * rem.clamp(max=31))) - 1)
    return win & keep


def emit(row):
    row.update(STAMP)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


sub_len = 1 << a.log2_nt
n_len = sub_len + (1 << 20)
d = torch.empty(n_len, dtype=torch.uint8, device="cuda")
devutil.fill_random_acgt(d, 1)
bits = cn.n_to_bits_dev(d)
del d
R = sub_len // 32
out = torch.empty(R, dtype=torch.int64, device="cuda")

# the bar: the two packed-domain streams with the same traffic
comp = timed(lambda: po.complement_dev(bits, sub_len, out=out), a.iters)
rc = timed(lambda: po.reverse_complement_dev(bits, sub_len, out=out), a.iters)
bar = rc[0] + (rc[2] - rc[1])
for start in (0, 32 * 1000, 17, (1 << 19) + 5):
    for rev in (False, True):
        po.subseq_dev(bits, n_len, start, sub_len, revcomp=rev, out=out)
        st, rv = torch.tensor([start], dtype=torch.int64, device="cuda"), torch.tensor([rev], device="cuda")
        for c0 in range(0, R, 1 << 24):  # verified in full, in chunks of 2^24 words
            assert torch.equal(out[c0 : c0 + (1 << 24)], torch_route(bits, st, sub_len, rv, c0, min(c0 + (1 << 24), R)).view(-1)), (start, rev, c0)
        ms = timed(lambda: po.subseq_dev(bits, n_len, start, sub_len, revcomp=rev, out=out), a.iters)
        emit({"op": "subseq", "nt": sub_len, "of_nt": n_len, "start": start, "phase": start % 32, "revcomp": rev, "ms": round(ms[0], 4), "min_ms": round(ms[1], 4),
              "max_ms": round(ms[2], 4), "GBs": round(sub_len / 2 / ms[0] / 1e6, 1), "complement_ms": round(comp[0], 4), "complement_min_ms": round(comp[1], 4),
              "complement_max_ms": round(comp[2], 4), "revcomp_ms": round(rc[0], 4), "revcomp_min_ms": round(rc[1], 4), "revcomp_max_ms": round(rc[2], 4),
              "within_bar": bool(ms[0] <= bar), "iters": a.iters})
del out

# windows
g = torch.Generator(device="cuda")
g.manual_seed(7)
for log2_n in (10, 16, 20):
    n = 1 << log2_n
    for region_len in (23, 101, 1000):
        Rw = (region_len + 31) // 32
        starts = torch.randint(0, sub_len - region_len + 1, (n,), dtype=torch.int64, device="cuda", generator=g)
        info = (torch.arange(n, dtype=torch.int64, device="cuda") & 1) * REVERSE + 2
        rec = torch.empty(n * Rw, dtype=torch.int64, device="cuda")
        rej = torch.zeros(1, dtype=torch.int64, device="cuda")
        for with_info in (False, True):
            rev = (info & REVERSE) != 0 if with_info else torch.zeros(n, dtype=torch.bool, device="cuda")
            fn = lambda: po.extract_dev(bits, sub_len, starts, region_len, info=info if with_info else None, out=rec, rejected=rej)  # noqa: E731
            fn()
            assert torch.equal(rec.view(n, Rw), torch_route(bits, starts, region_len, rev)) and int(rej.item()) == 0, (n, region_len, with_info)
            ms = timed(fn, a.iters)
            tm = timed(lambda: torch_route(bits, starts, region_len, rev), a.torch_iters)
            emit({"op": "extract", "nt": sub_len, "n": n, "region_len": region_len, "info": with_info, "ms": round(ms[0], 4), "min_ms": round(ms[1], 4),
                  "max_ms": round(ms[2], 4), "Mregions_s": round(n / ms[0] / 1e3, 1), "out_GBs": round(n * Rw * 8 / ms[0] / 1e6, 1),
                  "torch_ms": round(tm[0], 3), "vs_torch": round(tm[0] / ms[0], 1), "iters": a.iters, "torch_iters": a.torch_iters})

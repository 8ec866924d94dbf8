#!/usr/bin/env python3
"""Device-tier throughput of the open-reading-frame scan (packed_ops.orfs_dev) on one MI355X, product build, 2^30 nt by default.
Inputs: cnt_fill_random_acgt_dev data (a stop every ~21 codons of a lane: short runs, many entries) and random {A,C,G} (random
words with every T turned into G: no stop and no ATG on either strand) with a stop and a start of each strand planted every 2^16
nt (runs carried across eight tiles, a handful of entries).  Standard stops, ATG starts; min_len in {0, 300, 3000}; one strand
and both.  Every case is first checked at 2^22 nt against a numpy restatement of the definition.  One JSON row per case, printed
and appended to --out, every figure of a row taken in the same run:
  ms, min_ms, max_ms   median / extremes of --iters (>= 20) event-timed calls after a warm-up, the same buffers every call
  Gnts                 nucleotides per ns
  n                    entries of the call
  six_translate_ms     the six cnt_translate_dev calls of the whole sequence (what a caller runs today before they can begin to
                       look for stops), timed as one unit the same way
  vs_six_translate     six_translate_ms / ms
  find_ms              cnt_find_pattern_dev, 23 nt, three mismatches, both strands, on the same input
With --trace-only the script runs three scans of each input and nothing else: the workload of a rocprofv3 --kernel-trace --stats
run for the per-pass split."""
import argparse
import datetime
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import cute_nucleotides_amd as cn  # noqa: E402
from cute_nucleotides_amd import _lib, devutil, packed_ops as po  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-nt", type=int, default=30)
ap.add_argument("--log2-nt-check", type=int, default=22)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--min-lens", default="0,300,3000")
ap.add_argument("--trace-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orfs_bench.jsonl"))
a = ap.parse_args()
assert a.iters >= 20 and not _lib.is_lab_build()
STAMP = {"date": datetime.date.today().isoformat(), "build": "product"}
STOPS, ATG = _lib.CNT_ORF_STOPS_STANDARD, _lib.CNT_ORF_STARTS_ATG
GUIDE = "GATTACAGATTACAGATTACNGG"


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


def emit(row):
    row.update(STAMP)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


def packed_codes(text):
    return sum("ACTG".index(ch) << (2 * j) for j, ch in enumerate(text))


def sequence(kind, n_len):
    """the packed words of an input"""
    if kind == "acgt":
        d = torch.empty(n_len, dtype=torch.uint8, device="cuda")
        devutil.fill_random_acgt(d, 1)
        return cn.n_to_bits_dev(d)
    words = (n_len + 31) // 32
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    w = torch.randint(-(1 << 63), (1 << 63) - 1, (words,), dtype=torch.int64, device="cuda", generator=gen)
    w |= (w >> 1) & 0x5555555555555555  # code 2 (T) becomes 3 (G)
    # every 2^16 nt a forward stop, 2^14 nt on a forward start, then a reverse stop and a reverse start: six nucleotides each,
    # padded so that no other codon that overlaps them is a stop or a start (G in front, CC behind)
    for j, text in enumerate(("GTAACC", "GATGCC", "GTTACC", "GCATCC")):
        idx = torch.arange(512 * j, words, 2048, device="cuda")
        w[idx] = (w[idx] & ~0xFFF) | packed_codes(text)
    return w


def rc3_set(mask):
    return sum(1 << c for c in range(64) if (mask >> (((c >> 4) | (c & 0xC) | ((c & 3) << 4)) ^ 0x2A)) & 1)


def np_reference(words, n, starts, min_len, both):
    """the definition (include/cute_nt.h "ORF scan") on sorted position arrays: uint64 (pos, length, info)"""
    i = np.arange(n, dtype=np.uint64)
    s = ((words[(i >> np.uint64(5)).astype(np.int64)] >> (np.uint64(2) * (i & np.uint64(31)))) & np.uint64(3))
    c = s[:-2] | s[1:-1] << np.uint64(2) | s[2:] << np.uint64(4)
    parts = []
    for strand in (0, 1) if both else (0,):
        sm, am = (STOPS, starts) if strand == 0 else (rc3_set(STOPS), rc3_set(starts))
        sp = np.flatnonzero((np.uint64(sm) >> c) & np.uint64(1)).astype(np.int64)
        apos = np.flatnonzero((np.uint64(am) >> c) & np.uint64(1)).astype(np.int64)
        for lane in range(3):
            t = next(v for v in (n - 2, n - 1, n) if v % 3 == lane)
            bounds = np.concatenate([[lane - 3], sp[sp % 3 == lane], [t]]).astype(np.int64)
            lo, hi = bounds[:-1], bounds[1:]
            if starts:
                st = apos[apos % 3 == lane]
                j = np.searchsorted(st, lo, side="right") if strand == 0 else np.searchsorted(st, hi, side="left") - 1
                ok = (j >= 0) & (j < st.size)
                at = st[np.clip(j, 0, max(st.size - 1, 0))] if st.size else np.zeros_like(lo)
                ok &= (at > lo) & (at < hi)
                pos, length = (at, hi - at) if strand == 0 else (lo + 3, at - lo)
            else:
                ok, pos, length = np.ones(lo.size, dtype=bool), lo + 3, hi - lo - 3
            ok &= (length >= 3) & (length >= min_len)
            opening, closing = (lo < 0, hi >= n - 2) if strand == 0 else (hi >= n - 2, lo < 0)
            info = (lane if strand == 0 else (n - lane) % 3) | (_lib.CNT_FIND_REVERSE if strand else 0) | np.where(opening, _lib.CNT_ORF_OPEN_END, 0) | \
                np.where(closing, _lib.CNT_ORF_NO_STOP, 0)
            parts.append((2 * hi[ok] + strand, pos[ok], length[ok], info[ok]))
    order = np.argsort(np.concatenate([p[0] for p in parts]), kind="stable")
    return tuple(np.concatenate([p[j] for p in parts])[order].astype(np.uint64) for j in (1, 2, 3))


min_lens = [int(x) for x in a.min_lens.split(",")]
n_len, n_check = 1 << a.log2_nt, 1 << a.log2_nt_check
cap = n_len // 8
outs = [torch.empty(cap, dtype=torch.int64, device="cuda") for _ in range(3)]
count = torch.empty(1, dtype=torch.int64, device="cuda")
work = torch.empty(po.orfs_work_bytes(n_len), dtype=torch.uint8, device="cuda")


def scan(bits, n, min_len, both):
    return po.orfs_dev(bits, n, STOPS, ATG, min_len, both_strands=both, pos=outs[0], lens=outs[1], info=outs[2], count=count, work=work)


for kind in ("acgt", "acg_sparse"):
    bits = sequence(kind, n_len)
    if a.trace_only:
        for _ in range(3):
            scan(bits, n_len, 300, True)
        torch.cuda.synchronize()
        continue
    host = bits[: n_check // 32].cpu().numpy().view(np.uint64)
    for min_len in min_lens:
        for both in (False, True):
            scan(bits, n_check, min_len, both)
            n = int(count.item())
            want = np_reference(host, n_check, ATG, min_len, both)
            assert n == want[0].size <= cap and all(np.array_equal(o[:n].cpu().numpy().view(np.uint64), w) for o, w in zip(outs, want)), (kind, min_len, both, n)
    prot = torch.empty(n_len // 3 + 1, dtype=torch.uint8, device="cuda")
    six = timed(lambda: [po.translate_dev(bits, n_len, start, sub_len, rev, out=prot) for start, sub_len, rev in po._six_frames(n_len)], a.iters)
    pat = po.pattern_from_ascii(GUIDE)
    fwork = torch.empty(po.find_pattern_work_bytes(n_len, pat[2]), dtype=torch.uint8, device="cuda")
    find = timed(lambda: po.find_pattern_dev(bits, n_len, pat, 3, both_strands=True, pos=outs[0], info=outs[1], count=count, work=fwork), a.iters)
    del prot, fwork
    for min_len in (min_lens if kind == "acgt" else [300]):
        for both in (False, True):
            ms = timed(lambda: scan(bits, n_len, min_len, both), a.iters)
            n = int(count.item())
            assert n <= cap, (n, cap)
            emit({"op": "orfs", "input": kind, "stops": "TAA,TGA,TAG", "starts": "ATG", "min_len": min_len, "both_strands": both, "nt": n_len, "n": n,
                  "ms": round(ms[0], 4), "min_ms": round(ms[1], 4), "max_ms": round(ms[2], 4), "Gnts": round(n_len / ms[0] / 1e6, 2),
                  "six_translate_ms": round(six[0], 4), "six_translate_min_ms": round(six[1], 4), "six_translate_max_ms": round(six[2], 4),
                  "vs_six_translate": round(six[0] / ms[0], 3), "find_ms": round(find[0], 4), "find_min_ms": round(find[1], 4), "find_max_ms": round(find[2], 4),
                  "work_bytes": work.numel(), "iters": a.iters})
    del bits
    torch.cuda.empty_cache()

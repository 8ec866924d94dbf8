#!/usr/bin/env python3
"""Device-tier throughput of codon translation (packed_ops.translate_dev) on one MI355X, product build.  Every result is verified
in the run, before it is timed, against the same bytes computed with torch indexing and integer ops on the packed words.  One JSON
row per case, printed and appended to --out, every figure of a row taken in the same run:
  2^30 nt out of a 2^30 + 2^20 nt sequence, start in {0, 1, 2, 17}, forward and reversed, the default table and a custom one
    ms / min_ms / max_ms   median, fastest and slowest of --iters (>= 20) event-timed calls after a warm-up
    GBs                    bytes read + written per ns: 0.25 + 1/3 B per nt
    decode_ms (+ min / max), decode_GBs   cnt_bits_to_n_dev on 2^30 nt, the project's closest stream (packed words in, bytes
                           out: 1.25 B per nt) -- the bar
    vs_decode              GBs / decode_GBs: the share of decode's achieved bandwidth that translation reaches"""
import argparse
import datetime
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cute_nucleotides_amd as cn  # noqa: E402
from cute_nucleotides_amd import _lib, devutil, packed_ops as po  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--log2-nt", type=int, default=30)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "translate_bench.jsonl"))
a = ap.parse_args()
assert a.iters >= 20 and not _lib.is_lab_build()
STAMP = {"date": datetime.date.today().isoformat(), "build": "product"}


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
    return (x >> sh) & ~((torch.full_like(sh, -1) << (63 - sh)) << 1)


def torch_route(bits, start, sub_len, rev, table, j0, j1):
    """output bytes [j0, j1): gather the two words a codon may touch, funnel, take 6 bits, look them up"""
    j = torch.arange(j0, j1, dtype=torch.int64, device=bits.device)
    p = start + sub_len - 3 - 3 * j if rev else start + 3 * j
    iw, sh = p >> 5, 2 * (p & 31)
    c = (lsr(bits[iw], sh) | ((bits[(iw + 1).clamp(max=bits.numel() - 1)] << 1) << (63 - sh))) & 63
    if rev:
        c = ((c >> 4) | (c & 12) | ((c & 3) << 4)) ^ 0x2A
    return table[c]


def emit(row):
    row.update(STAMP)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


nt = 1 << a.log2_nt
n_len = nt + (1 << 20)
d = torch.empty(n_len, dtype=torch.uint8, device="cuda")
devutil.fill_random_acgt(d, 1)
bits = cn.n_to_bits_dev(d)

# the bar: decode of the same 2^30 nt, verified against the letters it came from
back = torch.empty(nt, dtype=torch.uint8, device="cuda")
cn.bits_to_n_dev(bits, nt, out=back)
assert torch.equal(back, d[:nt])
dec = timed(lambda: cn.bits_to_n_dev(bits, nt, out=back), a.iters)
dec_gbs = nt * 1.25 / dec[0] / 1e6
del d, back

custom = np.random.default_rng(5).integers(0, 256, 64).astype(np.uint8)
tables = {"standard": (None, torch.from_numpy(np.frombuffer(po.codon_table(1), dtype=np.uint8).copy()).cuda()), "custom": (custom, torch.from_numpy(custom).cuda())}
M = nt // 3
out = torch.empty(M, dtype=torch.uint8, device="cuda")
CHUNK = 1 << 24
for start in (0, 1, 2, 17):
    for rev in (False, True):
        for name, (tab, dtab) in tables.items():
            out.fill_(0)
            po.translate_dev(bits, n_len, start, nt, revcomp=rev, table=tab, out=out)
            for c0 in range(0, M, CHUNK):  # verified in full, in chunks of 2^24 bytes
                assert torch.equal(out[c0 : c0 + CHUNK], torch_route(bits, start, nt, rev, dtab, c0, min(c0 + CHUNK, M))), (start, rev, name, c0)
            ms = timed(lambda: po.translate_dev(bits, n_len, start, nt, revcomp=rev, table=tab, out=out), a.iters)
            gbs = nt * (0.25 + 1 / 3) / ms[0] / 1e6
            emit({"op": "translate", "nt": nt, "of_nt": n_len, "start": start, "revcomp": rev, "table": name, "ms": round(ms[0], 4), "min_ms": round(ms[1], 4),
                  "max_ms": round(ms[2], 4), "GBs": round(gbs, 1), "decode_ms": round(dec[0], 4), "decode_min_ms": round(dec[1], 4),
                  "decode_max_ms": round(dec[2], 4), "decode_GBs": round(dec_gbs, 1), "vs_decode": round(gbs / dec_gbs, 3), "iters": a.iters})

"""bench.py's host-side helpers, checked without a GPU: the numpy restatement it uses to spot-check the TIMED
packed buffer is the oracle's function, the crossover rule, the per-kernel statistics, and the table generator
reproduces DESIGN.md's round-2 table from the committed bench line."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_numpy_pack_is_the_oracle_on_whole_words(oracle):
    import bench

    rng = np.random.default_rng(3)
    for n_len in (32, 64, 32 * 1000):
        n = rng.integers(0, 256, n_len, dtype=np.uint8)
        assert np.array_equal(bench.numpy_pack(n), oracle.n_to_bits_bitextract(n))  # (byte>>1)&3 on whole words
        v = np.frombuffer(b"ACGTUacgtu", dtype=np.uint8)[rng.integers(0, 10, n_len)]
        assert np.array_equal(bench.numpy_pack(v), oracle.n_to_bits_lut(v))  # == n_to_bits_lut on the alphabet
    assert bench.numpy_pack(np.frombuffer(b"ATCG" * 8, dtype=np.uint8)).tolist() == [0xD8D8D8D8D8D8D8D8]  # n_to_bits.rs:414-415


def test_stats_and_crossover():
    import bench

    s = bench.stats_ms([3.0, 1.0, 2.0, 10.0])
    assert s == {"mean": 4.0, "median": 2.5, "min": 1.0, "max": 10.0, "n": 4}
    s = bench.stats_ms([float(x) for x in range(1, 21)])  # from 10 samples on: p10 / p90 (profiles/r04_decode_spread.md)
    assert s["p10"] == 3.0 and s["p90"] == 19.0 and s["n"] == 20 and s["min"] == 1.0 and s["max"] == 20.0
    host = {"2^12": {"n_to_bits_hip fresh out": 1.0, "bits_to_n_hip fresh out": 1.0},
            "2^20": {"n_to_bits_hip fresh out": 50.0, "bits_to_n_hip fresh out": 5.0},
            "2^30": {"n_to_bits_hip fresh out": 30.0, "bits_to_n_hip fresh out": 14.0}}
    cpu = {"2^12": {"n_to_bits_movemask": 60.0, "bits_to_n_shuffle": 30.0}, "2^20": {"n_to_bits_movemask": 40.0, "bits_to_n_shuffle": 70.0},
           "2^30": {"n_to_bits_movemask": 35.0, "bits_to_n_shuffle": 4.0}}
    x = bench.crossover(host, cpu)
    # ahead at 2^20 but behind again at 2^30: "ahead from" means ahead at every larger size too
    assert x["n_to_bits_hip vs n_to_bits_movemask"]["host_tier_ahead_from"] is None
    assert x["bits_to_n_hip vs bits_to_n_shuffle"]["host_tier_ahead_from"] == "2^30"
    assert bench.physical_cores(sorted(os.sched_getaffinity(0))) in (None,) + tuple(range(1, 4097))
    assert bench.gbs(8e12, 1000.0) == 8000.0


import pytest


DRIVER_RECORD = {"r06": "BENCH_r05.json"}  # the newest driver-timed line that existed when round 6's table was written


@pytest.mark.parametrize("tag", ["r02", "r03", "r04", "r05", "r06"])
def test_design_table_is_generated_from_the_committed_line(tag):
    line = os.path.join(ROOT, "profiles", tag + "_bench_final.json")
    j = json.load(open(line))
    # rounds 2-5 printed their table without the driver's column; from round 6 on the column names the driver record it quotes, so
    # that a newer BENCH_rNN.json appearing at the repo root (the driver writes one after every round) cannot change a committed table
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench", "design_table.py"), line, DRIVER_RECORD.get(tag, "none")], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr
    table = out.stdout.split("\n\n")[0]
    # the current round's table lives in DESIGN.md, the earlier rounds' in profiles/HISTORY.md (DESIGN.md as it stood then)
    doc = "DESIGN.md" if tag == "r06" else os.path.join("profiles", "HISTORY.md")
    design = open(os.path.join(ROOT, doc)).read()
    assert table in design, "%s's %s table is not the committed bench line's numbers: re-run bench/update_design_table.py" % (doc, tag)
    if tag == "r06":
        assert len(open(os.path.join(ROOT, "DESIGN.md")).read().splitlines()) <= 400  # a current-state document, not a log
    if tag in ("r03", "r04", "r05", "r06"):  # from round 3 on: the blocks VERDICT r02 asked for are on it, verified in-run
        assert j["codec5"]["verified"] is True and j["packed_ops"]["verified"] is True
        rag = j["configs"]["ragged: 2^30 - 19 nt (13 nt in the last word, zero-padded)"]
        assert rag["launches_per_call"] == 1 and rag["encode_vs_aligned_2p30"] < 1.01 and rag["decode_vs_aligned_2p30"] < 1.01
        h = j["host_tier"]
        # 0.85 on round 3's box, 0.72 on the box round 4's line came from with the same code (profiles/r04_ab_host_tier_vs_r03.jsonl:
        # both builds 22 ms in one process on a third box): the floor here is what no box has gone below
        assert h["pcie_ceiling"]["h2d_GiBs"] > 40 and min(v for k, v in h["frac_of_pcie_ceiling_at_2^30"].items() if "reused" in k) > 0.65
    # the line itself is internally consistent
    r = j["roofline"]
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["traffic_source"].startswith("measured by this run")
    assert abs(r["traffic"] / r["algorithmic_bytes_per_launch"] - 1) < 1e-3
    assert j["verified"] is True and j["n_gpus"] == 1 and j["ranks"][0]["pci_bus_id"]


def test_bench_refuses_cleanly_without_a_gpu():
    """no CPU fallback anywhere: on a box without a HIP device both launch forms of bench.py stop with one clear line
    (no traceback, nothing on stdout) -- including `--gpus N` without a launcher, which used to stop for a different
    reason ("needs a torch.distributed.run launch") before it had looked for devices at all"""
    import torch

    if torch.cuda.is_available():
        import pytest

        pytest.skip("this box has a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    for extra in ([], ["--gpus", "2"], ["--gpus", "8"]):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"] + extra,
                             capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert out.returncode != 0 and out.stdout.strip() == "", (extra, out.stdout[-300:])
        assert "no HIP device visible" in out.stderr and "Traceback" not in out.stderr, (extra, out.stderr[-600:])


def test_host_placement_reads_this_process():
    """bench.py's host_tier.placement block: NUMA nodes / huge-page share of a big array and the caller's CPU, from /proc and
    /sys -- must never raise, and on Linux it finds the array's pages (all of them touched here)."""
    import bench

    a = np.ones(64 << 20, dtype=np.uint8)
    p = bench.host_placement(a)
    assert isinstance(p, dict)
    if os.path.exists("/proc/self/numa_maps"):
        assert sum(p["pages_per_node"].values()) * 4096 >= a.nbytes // 2 and 0.0 <= p["huge_page_share"] <= 1.0
        assert p["caller_cpu"] >= 0
    assert bench.gpu_numa_node("0000:ff:1f.7") is None and bench.gpu_numa_node(None) is None  # no such device: no answer, no exception


def _fake_rows(n, chip=None, dup=None):
    rows = []
    for k in range(n):
        rows.append({"rank": k, "device_index": k, "pci_bus_id": "0000:%02x:00.0" % (0x05 + 0x10 * k), "numa_node": k // 4,
                     "uuid": "GPU-%032x" % (0xABC0 + k), "name": "AMD Instinct MI355X", "hbm_GiB": 287.98,
                     "chip": dict(chip or {"compute_units": 256, "lds_bytes_per_cu": 163840, "xcds": 8})})
    if dup is not None:
        rows[dup[1]]["uuid"], rows[dup[1]]["pci_bus_id"] = rows[dup[0]]["uuid"], rows[dup[0]]["pci_bus_id"]
    return rows


def test_first_contact_checklist_on_a_fake_eight_device_node():
    """no N > 1 path has met two real devices, so the first hardware line must diagnose itself.
    Fed an identity table of 8 visible devices (what device_row() builds from the C ABI), the `devices` block counts 8
    distinct ones over two NUMA nodes; a table in which two ranks sit on ONE device is refused unless the fold-onto-one-GPU
    test hook is on (then it is printed, labelled); a partitioned-mode device (fewer CUs / XCDs than an SPX MI355X) is
    named on the line; a short row list is refused."""
    import bench_measure as bm

    d = bm.first_contact_devices(_fake_rows(8), 8, False, visible=8, processes=1, control_plane=None)
    assert d["distinct"] == 8 and d["expected_distinct"] == 8 and d["shared_gpu_test_hook"] is False and d["numa_nodes"] == [0, 1]
    assert d["not_an_spx_mi355x"] == [] and d["data_path_collective"] is None and d["visible"] == 8 and d["processes"] == 1
    with pytest.raises(SystemExit, match="refusing to print a folded run as an 8-GPU line"):
        bm.first_contact_devices(_fake_rows(8, dup=(2, 5)), 8, False)
    d = bm.first_contact_devices(_fake_rows(8, dup=(2, 5)), 8, True)  # the test hook is on: printed, and says so
    assert d["distinct"] == 7 and d["shared_gpu_test_hook"] is True
    cpx = {"compute_units": 32, "lds_bytes_per_cu": 163840, "xcds": 1}
    d = bm.first_contact_devices(_fake_rows(8, chip=cpx), 8, False)
    assert len(d["not_an_spx_mi355x"]) == 8 and d["not_an_spx_mi355x"][3] == {"rank": 3, "pci_bus_id": "0000:35:00.0", "chip": cpx}
    with pytest.raises(SystemExit, match="7 report rows for 8 GPUs"):
        bm.first_contact_devices(_fake_rows(7), 8, False)
    # rows without a UUID fall back to the PCI address
    rows = _fake_rows(4)
    for r in rows:
        r["uuid"] = None
    assert bm.first_contact_devices(rows, 4, False)["distinct"] == 4


def test_free_hbm_check_fails_before_anything_is_allocated():
    import bench_measure as bm

    class FakeCuda:
        @staticmethod
        def mem_get_info(index):
            return ((200 << 30), (288 << 30)) if index == 0 else ((20 << 30), (288 << 30))  # device 1: another tenant holds it

    class FakeTorch:
        cuda = FakeCuda

    assert bm.require_free_hbm(FakeTorch, 0, 37 << 30, "the timed buffers") == {"free_GiB": 200.0, "total_GiB": 288.0}
    with pytest.raises(SystemExit, match="device 1 has 20.0 of 288.0 GiB of HBM free, the timed buffers needs 37.0 GiB"):
        bm.require_free_hbm(FakeTorch, 1, 37 << 30, "the timed buffers")


def test_static_traffic_is_labelled_as_an_n1_measurement_on_an_n_gpu_line():
    """the N > 1 lines quote profiles/hbm_traffic.json only under a label that says where it came from"""
    import bench_measure as bm

    t, src, live = bm.traffic_for_line(34, 8, allow_live=False)
    assert live is None and t["encode_bytes_per_launch"] > 0 and t["decode_bytes_per_launch"] > 0
    assert src.startswith("static, N = 1 measurement quoted on an N = 8 line: profiles/hbm_traffic.json") and "NOT measured by this run" in src
    t1, src1, _ = bm.traffic_for_line(34, 1, allow_live=False)
    assert src1.startswith("static: profiles/hbm_traffic.json") and t1 == t
    assert abs(t["encode_bytes_per_launch"] / (1.25 * 2**34) - 1) < 1e-3
    assert bm.traffic_for_line(26, 8, allow_live=False) == (None, None, None)  # the committed figure is for 2^34 nt only


def test_cpu_baseline_leg_for_the_n_gpu_lines(oracle):
    """bench.py's CPU leg as the N > 1 lines call it (faithful_tables=False): the all-core and one-thread figures of the AVX2
    ports, cores stated, without the reference-harness tables (those stay on the N = 1 line).  Runs here: it needs no GPU."""
    import bench

    if not oracle.port_cpu_ok():
        pytest.skip("host CPU lacks AVX2/BMI2")
    c = bench.cpu_baseline(1.0, faithful_tables=False)
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] == "port" and c["unit"] == "Gnt/s" and c["one_thread"]["value"] > 0
    assert "reference_faithful_40k_GiBs" not in c and "N = 1 line" in c["reference_faithful_tables"]
    assert c["cores_detail"]["threads_timed"] == c["cores"] and "sample" in c


def test_the_pmc_child_of_an_n_gpu_line_sees_one_device():
    """the live-traffic leg of an N > 1 line runs rocprofv3 over a one-device child: rank 0's device, hidden at the ROCr level so
    that the profiler's own agent enumeration is restricted too; visibility lists the parent was launched under are resolved"""
    import bench_measure as bm

    gone = {"CUDA_VISIBLE_DEVICES": None}  # never inherited: it would be applied on top of the narrowed set
    assert bm.one_device_env({}, 0) == dict(gone, ROCR_VISIBLE_DEVICES="0", HIP_VISIBLE_DEVICES="0")
    assert bm.one_device_env({}, 5) == dict(gone, ROCR_VISIBLE_DEVICES="5", HIP_VISIBLE_DEVICES="0")
    assert bm.one_device_env({"HIP_VISIBLE_DEVICES": "4,5,6,7"}, 2) == dict(gone, ROCR_VISIBLE_DEVICES="6", HIP_VISIBLE_DEVICES="0")
    assert bm.one_device_env({"ROCR_VISIBLE_DEVICES": "2,3", "HIP_VISIBLE_DEVICES": "1,0"}, 0) == dict(gone, ROCR_VISIBLE_DEVICES="3", HIP_VISIBLE_DEVICES="0")
    assert bm.one_device_env({"ROCR_VISIBLE_DEVICES": "GPU-abc,GPU-def"}, 1) == dict(gone, ROCR_VISIBLE_DEVICES="GPU-def", HIP_VISIBLE_DEVICES="0")
    assert bm.one_device_env({"HIP_VISIBLE_DEVICES": "GPU-abc,GPU-def"}, 1) == dict(gone, HIP_VISIBLE_DEVICES="GPU-def")  # UUIDs: filter in HIP
    # HIP on ROCm honours CUDA_VISIBLE_DEVICES too -- with HIP_VISIBLE_DEVICES unset it is the index list (rank 0 of a
    # parent started with CUDA_VISIBLE_DEVICES=4,5 is physical GPU 4, not 0), HIP_VISIBLE_DEVICES wins when both are set
    assert bm.one_device_env({"CUDA_VISIBLE_DEVICES": "4,5"}, 0) == dict(gone, ROCR_VISIBLE_DEVICES="4", HIP_VISIBLE_DEVICES="0")
    assert bm.one_device_env({"CUDA_VISIBLE_DEVICES": "4,5", "ROCR_VISIBLE_DEVICES": "0,1,2,3,7,6"}, 1) == dict(gone, ROCR_VISIBLE_DEVICES="6", HIP_VISIBLE_DEVICES="0")
    assert bm.one_device_env({"CUDA_VISIBLE_DEVICES": "4,5", "HIP_VISIBLE_DEVICES": "2"}, 0) == dict(gone, ROCR_VISIBLE_DEVICES="2", HIP_VISIBLE_DEVICES="0")
    env = bm.apply_env({"CUDA_VISIBLE_DEVICES": "4,5", "PATH": "/bin"}, bm.one_device_env({"CUDA_VISIBLE_DEVICES": "4,5"}, 1))
    assert env == {"PATH": "/bin", "ROCR_VISIBLE_DEVICES": "5", "HIP_VISIBLE_DEVICES": "0"}


@pytest.mark.parametrize("n_len, shards, first_word", [(32 * 1000 + 13, 1, 0), (32 * ((1 << 18) + 4096), 1, 0), (32 * (1 << 17) + 5, 3, 1 << 20)])
def test_dump_outputs_writes_the_callers_arrays(oracle, tmp_path, n_len, shards, first_word):
    """--dump-outputs on CPU tensors: every word when there are few, a fixed seeded sample of 2^18 / shards words (first and
    last included) when there are more; the files restate the packed words exactly and the decoded bytes, -1 past the end,
    under their global word indices; N shards of a run stay within the 64 MB budget together; the same seed writes the same
    files."""
    import torch

    import bench

    n = oracle.fill_random_acgt(n_len, 9)
    words = oracle.n_to_bits_lut(n)
    d_packed, d_out = torch.from_numpy(words.view(np.int64).copy()), torch.from_numpy(n.copy())
    prefix = "" if shards == 1 else "shard1_"
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), torch, d_packed, d_out, n_len, 0x5EED, first_word, shards, prefix)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == [prefix + f for f in ("decoded.npy", "packed_words.npy", "words_index.npy")]
    assert shards * sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    idx = np.load(tmp_path / "a" / (prefix + "words_index.npy"))
    pk = np.load(tmp_path / "a" / (prefix + "packed_words.npy"))
    dec = np.load(tmp_path / "a" / (prefix + "decoded.npy"))
    assert idx.dtype == pk.dtype == np.float64 and dec.dtype == np.float32
    k = min(words.size, bench.DUMP_WORDS // shards)
    assert idx.shape == (k,) and pk.shape == (k, 2) and dec.shape == (k, 32)
    w = idx.astype(np.int64) - first_word
    assert w[0] == 0 and w[-1] == words.size - 1 and np.all(np.diff(w) > 0)
    assert np.array_equal(pk[:, 0].astype(np.uint64) | (pk[:, 1].astype(np.uint64) << np.uint64(32)), words[w])
    pos = w[:, None] * 32 + np.arange(32)
    assert np.array_equal(dec, np.where(pos < n_len, n[np.minimum(pos, n_len - 1)].astype(np.float32), np.float32(-1)))

"""bench.py's contract line (driver contract + roofline / cpu_baseline objects), on a down-sized workload,
and a rehearsal of its N>1 code path (RCCL group, panel pipeline, breakdown legs) with a world of one."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, **env_extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29519", **env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--M", "65536", "--steps", "3", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    # stdout carries the contract line and NOTHING else (RCCL's version banner, which the library prints to stdout, included: bench.py
    # points fd 1 at stderr and writes the line through a private duplicate of the original stdout)
    assert r.stdout.count("\n") == 1 and r.stdout.startswith("{"), repr(r.stdout[:200])
    return json.loads(r.stdout)


def test_single_gpu_line():
    d = _run("--cpu-rows", "16384", "--check")
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None and d["unit"] == "GFLOP/s"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "rate_kind" in r and "split_mode" in r and r["tile_cols_in_force"] == 128
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c
    assert c["single_thread"]["cores"] == 1 and c["single_thread"]["value"] > 0 and "march" in c["sample"]
    assert d["ms_per_step_ref_protocol"] >= d["device_ms_per_step"] * 0.9      # util.h:141-151: 20 individually synchronised runs
    assert d["check"]["bitwise_equal_rows"] == d["check"]["rows"]
    assert abs(d["value"] - 2.0 * d["config"]["nnz"] * d["config"]["N"] / (d["ms_per_step"] * 1e-3) / 1e9) / d["value"] < 1e-3
    assert "l2_fabric" in r["bound_detail"] and "frac_of_measured_copy_6290" in r
    # the other single-GPU BASELINE configurations ride in the same line (timed after the headline's region)
    also = d["also"]
    assert set(also) == {"C2", "C4", "C1_N1024", "LONG_ROWS", "AM32"}
    for k, e in also.items():
        assert "error" not in e, (k, e)
        for key in ("config", "ms_per_step", "value", "roofline", "steps", "summation_order"):
            assert key in e, (k, key)
        assert e["ms_per_step"] > 0 and e["value"] > 0 and e["steps"] == 3 and e["summation_order"].startswith("exact")
        ro = e["roofline"]
        for key in ("bound", "achieved", "peak", "frac", "bytes_min", "traffic", "traffic_source"):
            assert key in ro, (k, key)
        if ro["bound"] == "chain":       # lower is better: floor / achieved
            assert abs(ro["frac"] - ro["floor_cycles"] / ro["cycles_per_nonzero"]) < 1e-3 and ro["achieved"] == ro["cycles_per_nonzero"]
        elif ro["frac"] is None:         # only the counter-less cache-resident form may decline to claim a fraction (this down-sized B is 4 MiB)
            assert ro["bound"] == "l2_gather" and ro["achieved"] > ro["peak"] and "frac_note" in ro
            continue
        else:
            assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-3
        assert 0 < ro["frac"] <= 1.0, (k, ro["frac"])          # a fraction above 1 is not a roofline fraction
    # the hub kernel rides in the driver's line, on the bound that is its own: the longest row's dependent chain
    am = also["AM32"]
    assert am["roofline"]["bound"] == "chain" and am["roofline"]["kernel"].startswith("mi::spmm_hub") and am["options"]["n_hub_rows"] >= 1
    assert am["roofline"]["longest_row"] == am["options"]["max_row_nnz"] and "N=32" in am["config"]
    # a cache-resident B is never priced against HBM on gather-model bytes
    lr = also["LONG_ROWS"]["roofline"]
    assert lr["bound"] in ("fabric", "l2_gather") and lr["b_bytes"] <= 256 << 20 and lr["achieved_alg"] > 0
    assert also["C4"]["roofline"]["bound"] == "mfma" and also["C4"]["roofline"]["block_items"]["n_block_groups"] == 65536 // 16
    # (down-sized here: M = 65 536 makes C2's B 32 MiB and C1_N1024's exactly 256 MiB -- cache-resident by the rule above; at the driver's size both are "hbm")
    assert also["C2"]["roofline"]["bound"] in ("hbm", "l2_gather") and also["C1_N1024"]["roofline"]["bound"] in ("hbm", "l2_gather")
    assert "N=1024" in also["C1_N1024"]["config"] and "N=256" in also["C4"]["config"]
    assert also["LONG_ROWS"]["options"]["n_col_strips"] >= 1 and also["LONG_ROWS"]["options"]["n_medium_rows"] > 0


def test_dump_outputs_is_the_timed_steps_c(tmp_path):
    """--dump-outputs DIR: the C the timed steps computed, as float32 rows with their indices (float64).  A C above the byte
    budget (here 64 MiB) is a seeded row sample, the same rows on every run; each sampled row equals the oracle's bit for bit."""
    import argparse

    import numpy as np

    sys.path.insert(0, ROOT)
    import bench
    from oracle import oracle

    d = _run("--N", "256", "--no-also", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "out"))
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    C = np.load(tmp_path / "out" / "C_sample.npy")
    rows = np.load(tmp_path / "out" / "C_sample_rows.npy")
    assert C.dtype == np.float32 and rows.dtype == np.float64
    assert C.nbytes + rows.nbytes <= 64 * 10**6
    assert C.shape == (bench.DUMP_BUDGET_BYTES // (4 * 256), 256) and rows.shape == (C.shape[0],)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 65536
    a = argparse.Namespace(mode="weak", N=256, M=65536, config="C1")
    _, M, _, _, ptr, idx, vals, B = bench.build_inputs(a, 1, 0)
    r = rows.astype(np.int64)
    deg = np.diff(ptr)[r]
    sp = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    take = np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in r])
    exp = oracle.spmm_omp(sp, idx[take], vals[take], B)
    assert np.array_equal(C.view(np.uint32), exp.view(np.uint32))


@pytest.mark.parametrize("exchange", ["allgather", "direct", "peer2d", "peer_store"])
def test_multi_gpu_path_rehearsal(exchange):
    d = _run("--rehearse-multi", "--no-cpu-baseline", "--check", "--panels", "3", "--exchange", exchange)
    assert d["check"]["bitwise_equal_rows"] == d["check"]["rows"]
    b = d["multi_gpu_breakdown"]
    assert "error" not in b and b["compute_only_ms"] > 0 and b["exchange_only_ms"] > 0 and b["exchange"] == exchange
    assert (b["staging_bytes"] > 0) == (exchange not in ("peer2d", "peer_store")) and "strong_reference_ms" in d and d["strong_reference_ms"] > 0
    assert d["cpu_baseline"] is None
    assert d["exchange"] == exchange and d["exchange_selection"]["rule"] == f"fixed by --exchange {exchange}"
    assert abs(d["speedup_vs_one_gpu"] - d["strong_reference_ms"] / d["ms_per_step"]) < 2e-3
    r = d["roofline"]        # N>1: the same per-GPU kernel, timed on the compute-only leg
    assert r["bound"] == "hbm" and r["traffic"] is None and abs(r["kernel_ms"] - b["compute_only_ms"]) < 1e-3
    # the link probe ran (a world of one has no peer: every rate 0, no bound) and left a complete C behind (--check above)
    lk = b["links"]
    assert "error" not in lk and lk["per_peer_GBs"] == [0.0] and lk["all_peers_GBs"] == 0.0 and lk["link_type"] == ["unknown"] and lk["link_bound_ms"] is None


def test_multi_gpu_default_is_safe_first_auto():
    """`bench.py --gpus N` with default flags (what the driver runs): the contract line is first measured on the RCCL all-gather
    (the safe schedule) and kept in hand, then direct / peer2d / peer_store are tried under the watchdog; the line says which
    schedule it was finally measured on and carries the all-gather's figures beside it."""
    d = _run("--rehearse-multi", "--no-cpu-baseline", "--check", "--panels", "3")
    assert d["check"]["bitwise_equal_rows"] == d["check"]["rows"]
    sel = d["exchange_selection"]
    assert sel["safe_schedule"] == "allgather" and sel["safe_schedule_ms_per_step"] > 0 and "safe-first" in sel["rule"]
    tuning = sel["exchange_tuning_ms_per_step"]
    assert {"allgather", "direct", "peer2d", "peer_store"} <= set(tuning) and all(tuning[k] > 0 for k in ("allgather", "direct", "peer2d", "peer_store"))
    assert d["exchange"] in ("allgather", "direct", "peer2d", "peer_store") and d["multi_gpu_breakdown"]["exchange"] == d["exchange"]
    if d["exchange"] != "allgather":                 # re-measured with the contract protocol, and faster than the safe schedule
        assert d["ms_per_step"] < sel["safe_schedule_ms_per_step"] and (d["exchange"] + " (contract protocol)") in tuning
    else:
        assert abs(d["ms_per_step"] - sel["safe_schedule_ms_per_step"]) < 1e-3
    assert d["strong_reference_ms"] > 0 and abs(d["speedup_vs_one_gpu"] - d["strong_reference_ms"] / d["ms_per_step"]) < 2e-3
    assert "exchange_watchdog" not in d


def test_multi_gpu_candidate_that_throws_is_dropped():
    d = _run("--rehearse-multi", "--no-cpu-baseline", "--panels", "3", MI_SPMM_FORCE_FAIL_EXCHANGE="direct")
    tuning = d["exchange_selection"]["exchange_tuning_ms_per_step"]
    assert tuning["direct"] is None and tuning["allgather"] > 0 and d["exchange"] != "direct" and "exchange_watchdog" not in d


def test_multi_gpu_candidate_that_hangs_still_yields_the_line_in_hand():
    """A schedule that neither finishes nor throws (forced: MI_SPMM_FORCE_HANG_EXCHANGE) must not cost the measurement: the
    per-rank watchdog prints the all-gather line it has in hand, says what hung, and the process leaves (exit code 0: the
    line is a complete measurement)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29519", MI_SPMM_FORCE_HANG_EXCHANGE="peer2d", MI_SPMM_WATCHDOG_S="25")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--M", "65536", "--steps", "3", "--warmup", "1", "--rehearse-multi",
                        "--no-cpu-baseline", "--panels", "3"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout + r.stderr
    d = json.loads(lines[0])
    assert r.returncode == 0, r.stderr
    assert d["exchange"] == "allgather" and "peer2d" in d["exchange_watchdog"]["fired_in"]
    tuning = d["exchange_selection"]["exchange_tuning_ms_per_step"]
    assert tuning["allgather"] > 0 and tuning["direct"] > 0 and "peer2d" not in tuning      # direct was tried before the hang
    assert d["ms_per_step"] > 0 and d["n_gpus"] == 1 and d["steps"] == 3
    assert "watchdog" in r.stderr and "hanging on purpose" in r.stderr
    # with MI_SPMM_WATCHDOG_EXIT the same stop can be made to read as a failure
    env["MI_SPMM_WATCHDOG_EXIT"] = "4"
    env["MI_SPMM_FORCE_HANG_EXCHANGE"] = "direct"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--M", "65536", "--steps", "2", "--warmup", "1", "--rehearse-multi",
                        "--no-cpu-baseline", "--panels", "3"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 4 and len([l for l in r.stdout.splitlines() if l.startswith("{")]) == 1


def test_multi_gpu_fallback_to_the_python_schedule():
    """If the C-ABI step cannot be set up on some rank, every rank agrees to run the same schedule stated in Python over
    torch.distributed (hpc_amd/dist.py ColumnShardedSpMM) and the line says so."""
    d = _run("--rehearse-multi", "--no-cpu-baseline", "--check", "--panels", "3", MI_SPMM_FORCE_PY_DIST="1")
    assert d["check"]["bitwise_equal_rows"] == d["check"]["rows"]
    b = d["multi_gpu_breakdown"]
    assert "error" not in b and "fallback" in b["step_path"] and b["exchange"] == "allgather"


def test_driver_launch_line_two_ranks_sharing_the_gpu():
    """The driver's N=2 command (python -m torch.distributed.run ... bench.py --gpus 2), both ranks on cuda:0
    over gloo (MI_SPMM_SHARE_GPU=1: RCCL refuses two ranks on one device).  One JSON line, from rank 0."""
    env = dict(os.environ, MI_SPMM_SHARE_GPU="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29633", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "2", "--warmup", "1", "--M", "65536", "--check"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["N"] == 256 and d["config"]["cols_per_gpu"] == 128
    assert "rehearsal" in d and d["check"]["bitwise_equal_rows"] == d["check"]["rows"]
    # ranks sharing a GPU cannot use RCCL: the safe schedule is peer2d (IPC copies + host barriers), the candidate peer_store
    sel = d["exchange_selection"]
    assert sel["safe_schedule"] == "peer2d" and set(sel["exchange_tuning_ms_per_step"]) >= {"peer2d", "peer_store"}
    assert "error" not in d["multi_gpu_breakdown"] and d["multi_gpu_breakdown"]["exchange"] == d["exchange"] and d["exchange"] in ("peer2d", "peer_store")
    assert d["strong_reference_ms"] > 0 and d["speedup_vs_one_gpu"] > 0
    assert abs(d["value"] - 2.0 * d["config"]["nnz"] * 256 / (d["ms_per_step"] * 1e-3) / 1e9) / d["value"] < 1e-3
    # SURVEY.md H3 / VERDICT r4 #2: the first N > 1 line explains itself -- per-peer and all-peers copy rates, link type, hop count, and the exchange time
    # those rates allow, beside ms_per_step.  (Two ranks on one GPU: the copies never leave the device; the code path is what is covered.)
    lk = d["multi_gpu_breakdown"]["links"]
    assert "error" not in lk, lk
    assert lk["per_peer_GBs"][0] == 0.0 and lk["per_peer_GBs"][1] > 10.0 and lk["all_peers_GBs"] > 10.0      # rank 0's view: itself 0, its one peer measured
    assert lk["link_type"] == ["unknown", "unknown"] and lk["hops"] == [-1, -1] and "share one GPU" in lk["note"]
    assert lk["link_bound_ms"] > 0 and lk["all_peers_GBs_min_over_ranks"] > 0 and lk["per_peer_GBs_min_over_ranks"] > 0
    assert abs(lk["link_bound_ms"] - 65536 * 128 * 4 / (lk["all_peers_GBs_min_over_ranks"] * 1e9) * 1e3) < 0.05 * lk["link_bound_ms"] + 1e-3


def test_link_probe_that_hangs_costs_the_probe_not_the_line():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29519", MI_SPMM_FORCE_HANG_EXCHANGE="link_probe", MI_SPMM_WATCHDOG_S="25")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--M", "65536", "--steps", "2", "--warmup", "1", "--rehearse-multi",
                        "--no-cpu-baseline", "--panels", "3", "--exchange", "allgather", "--no-strong-reference"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.returncode == 0, r.stdout + r.stderr
    d = json.loads(lines[0])
    assert "link probe" in d["watchdog_fired"] and d["ms_per_step"] > 0 and d["multi_gpu_breakdown"]["compute_only_ms"] > 0
    assert "links" not in d["multi_gpu_breakdown"]


def test_driver_launch_line_two_ranks_with_a_candidate_that_hangs():
    """The same two-rank launch with the candidate schedule hanging on BOTH ranks: each rank's watchdog fires, rank 0 prints
    the peer2d line it has in hand, torch.distributed.run sees two clean exits."""
    env = dict(os.environ, MI_SPMM_SHARE_GPU="1", MI_SPMM_FORCE_HANG_EXCHANGE="peer_store", MI_SPMM_WATCHDOG_S="25")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29641", os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "2", "--warmup", "1", "--M", "65536"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout + r.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["exchange"] == "peer2d" and "peer_store" in d["exchange_watchdog"]["fired_in"]
    assert d["ms_per_step"] > 0 and d["config"]["N"] == 256

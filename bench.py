#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X KMP packet-payload matcher.

Workload (BASELINE.json configs[1], per GPU): 1 000 000 synthetic UDP payloads of 1500 B
(bytes uniform over a..z, NUL-free), one 16-byte pattern planted in ~10 % of the packets;
generator: include/kmp_synth.h, seed 1234.  A "step" is one full pass of the hot path over that
arena (scan kernel + partial-count reduce, then the cross-GPU count sum), inputs resident in HBM.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...   (N > 1)

Rank 0 prints ONE JSON line (contract in the task statement) with an extra object:
  roofline     -- HBM roofline of the scan kernel: algorithmic bytes (sum of payload lengths of
                  one launch) / average launch duration measured with HIP events on the launch
                  stream during the timed steps, against 8.0 TB/s.
A plain run stops there.  --full adds, after the timed steps (rank 0, N == 1 only):
  cpu_baseline  -- the CPU restatement of openmp_data.c:126-178 (oracle/, "port") timed on the
                   host cores on the same arena (--no-cpu-baseline leaves it out);
  extra_configs -- the other BASELINE configs and the dense-candidate / adversarial inputs, each
                   count-checked and timed on its own (--no-extra leaves them out).
--dump-outputs DIR writes what the last timed step computed, the per-pattern match counts after
the reduce over ranks, as DIR/counts.npy (float64, one entry per pattern).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s spec
NEEDLE = b"NEEDLE_16B_PATRN"
PAYLOAD_LEN = 1500
SEED = 1234


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def host_cores() -> int:
    """CPU threads this process may really use: the scheduler affinity capped by the cgroup CPU
    quota (a GPU box exposes all 256 logical CPUs but grants a 16-CPU share)."""
    n = os.cpu_count() or 1
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, -(-int(txt[0]) // int(txt[1]))))
            else:
                q = int(txt[0])
                p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, -(-q // p)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


def cpu_model() -> str:
    """'model name' of the host CPU (print nproc and the CPU model beside the CPU figure)."""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.lower().startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine() or "unknown"


def self_launch(n_gpus: int) -> int:
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves, one process per GPU, as
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`
    (mpirun -np N of mpi_dumping.c:29-31).  This parent never touches the GPU (no torch import, no HIP call): the ranks
    are fresh child processes, their stdout -- rank 0's ONE JSON line -- is ours, and their exit code is ours."""
    import socket
    import subprocess
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC: RCCL across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log(f"bench.py: WORLD_SIZE is not set; starting {n_gpus} ranks: {' '.join(cmd)}")
    return subprocess.run(cmd, env=env).returncode


def extra_configs(m, dev, passes, headline, sample97):
    """The other BASELINE configs and the rows VERDICT asks to see through a driver-timed command: each leg is
    count-checked first, then `passes` back-to-back passes are timed with HIP events around the scan launches
    (kmpgpu_profile_begin/end).  Returns a list of dicts; algorithmic bytes = sum of payload lengths, one read."""
    import torch

    import multithreading_string_matching_amd as K
    from multithreading_string_matching_amd.matcher import (KERNEL_AUTO, KERNEL_GENERAL, MODE_AUTOMATON, MODE_FILTER, OPT_FUSED, OPT_KERNEL,
                                                            OPT_MODE)

    data = os.path.join(ROOT, "tests", "golden", "data")
    pats97 = K.load_patterns(os.path.join(data, "strings.txt"))
    out = []

    def timed(name, config, payload_bytes, check, note=None, settle=200):      # settle: as for the headline, the clocks have dropped during the count check
        for _ in range(settle):
            m.scan_enqueue()
        m.sync()
        m.profile_begin(passes * 8)
        for _ in range(passes):
            m.scan_enqueue()
        ms = m.profile_end(passes * 8)
        per_pass = float(ms.sum()) / passes
        gbs = payload_bytes / (per_pass * 1e-3) / 1e9
        row = {"name": name, "config": config, "ms": round(per_pass, 5), "launches_per_pass": int(round(len(ms) / passes)),
               "algorithmic_bytes": int(payload_bytes), "achieved_GBps": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4),
               "count_check": check}
        if note:
            row["note"] = note
        out.append(row)
        log(f"extra {name}: {per_pass * 1e3:.1f} us/pass, {gbs:.0f} GB/s, frac {gbs / HBM_PEAK_GBS:.3f} ({check})")

    def device_arena(lens, fixed_len, n, sp):
        off, ln, nbytes = K.arena_layout(lens, fixed_len, n)
        d_a = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        d_o = torch.from_numpy(off.astype(np.int64)).to(dev)
        d_l = torch.from_numpy(ln.astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        m.synth_fill(d_a, d_o, d_l, sp)
        m.sync()
        return d_a, d_o, d_l, int(ln.astype(np.int64).sum())

    # (1) strings.txt (97 patterns) over the headline arena: the multi-pattern outer loop serial.c:154 at HBM scale, fused pass
    d_arena, d_off, d_len, n, plen = headline
    m.set_option(OPT_FUSED, 0)
    m.set_patterns(pats97)
    m.attach_arena(d_arena, d_off, d_len)
    per_pattern, _ = m.scan()                       # 97 single-pattern streaming passes: an independent implementation
    m.set_option(OPT_FUSED, 2)
    m.attach_arena(d_arena, d_off, d_len)
    fused, _ = m.scan()
    if fused.tolist() != per_pattern.tolist():
        raise SystemExit("extra strings.txt x 1M x 1500 B: fused counts differ from the per-pattern passes")
    check = "fused == 97 single-pattern passes over the full arena"
    if sample97 is not None:
        ns, want = sample97
        m.attach_arena(d_arena, d_off[:ns], d_len[:ns])
        got, _ = m.scan()
        if got.tolist() != want:
            raise SystemExit("extra strings.txt: fused counts on the oracle sample differ from the oracle")
        check += f"; == oracle on the first {ns} packets"
        m.attach_arena(d_arena, d_off, d_len)
    timed("strings_txt_97_x_1m_1500B_fused", "BASELINE configs[2] pattern set (strings.txt, 97 tokens, 88 distinct) over configs[1]'s arena, "
          "ONE read of the arena (kmp_scan_multi_kernel)", n * plen, check)
    del d_arena, d_off, d_len, headline
    m.set_patterns([NEEDLE])
    m.attach_arena(torch.zeros(0, dtype=torch.uint8, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                   torch.zeros(0, dtype=torch.int32, device=dev))
    torch.cuda.empty_cache()

    # (2) BASELINE configs[4], per-GPU shape: 1 M payloads, lengths 64..9000 B Zipf(1.1) over the length ranks
    rng = np.random.default_rng(4)
    ranks = np.arange(1, 9000 - 64 + 2)
    pz = 1.0 / ranks ** 1.1
    pz /= pz.sum()
    nz = 1_000_000
    zl = (64 + rng.choice(len(ranks), size=nz, p=pz)).astype(np.uint32)
    sp = K.SynthParams.make(seed=SEED, needle=NEEDLE, plant_permille=100)
    d_a, d_o, d_l, pb = device_arena(zl, 0, nz, sp)
    m.set_patterns([NEEDLE])
    m.attach_arena(d_a, d_o, d_l)
    want = K.synth_count_planted(sp, nz, 0, lens=zl)
    got, _ = m.scan()
    if int(got[0]) != want:
        raise SystemExit(f"extra zipf: count {int(got[0])} != planted {want}")
    timed("zipf_1m_64_9000B", "BASELINE configs[4] per-GPU shape: 1 M payloads, 64..9000 B Zipf(1.1), one 16-byte pattern in ~10 % of packets, "
          "byte-balanced wavefront ranges (kmp_scan_packed_kernel)", pb, f"count == planted ({want})")
    # the same arena under the 97 patterns
    m.set_option(OPT_FUSED, 0)
    m.set_patterns(pats97)
    m.attach_arena(d_a, d_o, d_l)
    per_pattern, _ = m.scan()
    m.set_option(OPT_FUSED, 2)
    m.attach_arena(d_a, d_o, d_l)
    fused, _ = m.scan()
    if fused.tolist() != per_pattern.tolist():
        raise SystemExit("extra zipf x 97: fused counts differ from the per-pattern passes")
    timed("zipf_1m_64_9000B_x_strings_txt_97_fused", "the same arena, strings.txt (97 patterns), fused pass", pb,
          "fused == 97 single-pattern passes")
    del d_a, d_o, d_l
    torch.cuda.empty_cache()

    # (3) BASELINE configs[2]: very_big_udp.pcap x strings.txt (and big_udp.pcap, whose counts are not all zero)
    with open(os.path.join(ROOT, "tests", "golden", "fixture_counts.json")) as f:
        golden = json.load(f)["fixtures"]
    for fx in ("very_big_udp.pcap", "big_udp.pcap"):
        a = K.HostArena.from_pcap(os.path.join(data, fx), "udp")
        m.set_patterns(pats97)
        m.load_arena(a)
        got, _ = m.scan()
        if got.tolist() != golden[f"{fx}:udp"]["counts"]:
            raise SystemExit(f"extra {fx}: counts differ from the golden vector (serial.c's)")
        timed(f"{fx.split('.')[0]}_x_strings_txt_97", f"BASELINE configs[2]: {fx} ({a.n_pkts} payloads) x strings.txt, fused pass",
              a.payload_bytes, "== golden counts of serial.c (SURVEY App. B)",
              note="1.3 MB / 0.6 MB of payload: cache-resident and launch-latency-bound, the HBM fraction is not meaningful here")

    # (4) dense candidates in small packets: 64-byte payloads, needle in 10 % of them; lengths 34..328 B (very_big_udp.pcap's range)
    for name, lo, hi, nn in (("small_64B_needle_10pct", 64, 64, 12_000_000), ("small_34_328B_needle_10pct", 34, 328, 4_000_000)):
        lens = np.random.default_rng(5).integers(lo, hi + 1, size=nn).astype(np.uint32)
        d_a, d_o, d_l, pb = device_arena(lens, 0, nn, sp)
        m.set_patterns([NEEDLE])
        m.attach_arena(d_a, d_o, d_l)
        want = K.synth_count_planted(sp, nn, 0, lens=lens)
        got, _ = m.scan()
        if int(got[0]) != want:
            raise SystemExit(f"extra {name}: count {int(got[0])} != planted {want}")
        timed(name, f"{nn} payloads of {lo}..{hi} B, one 16-byte pattern in ~10 % of packets (a candidate in most 1 KiB chunks)", pb,
              f"count == planted ({want})")
        if lo == hi:
            # the same 64-byte payloads under the 97 patterns: sixteen packet starts per 1 KiB chunk in the fused pass
            m.set_option(OPT_FUSED, 0)
            m.set_patterns(pats97)
            m.attach_arena(d_a, d_o, d_l)
            per_pattern, _ = m.scan()
            m.set_option(OPT_FUSED, 2)
            m.attach_arena(d_a, d_o, d_l)
            fused, _ = m.scan()
            if fused.tolist() != per_pattern.tolist():
                raise SystemExit("extra 64 B x 97: fused counts differ from the per-pattern passes")
            timed("small_64B_x_97_fused", f"the same {nn} payloads of {lo} B, strings.txt (97 patterns), fused pass", pb, "fused == 97 single-pattern passes")
        del d_a, d_o, d_l
        torch.cuda.empty_cache()

    # (5) worst cases for a filter-then-confirm scan: text that is a candidate everywhere
    na, la = 200_000, 1500
    for name, span, pat, closed in (("adversarial_all_a_x_a16", 1, b"a" * 16, na * (la - 15)),
                                    ("adversarial_all_a_x_a15b", 1, b"a" * 15 + b"b", 0),
                                    ("adversarial_all_a_x_a40", 1, b"a" * 40, na * (la - 39)),
                                    ("adversarial_ab_x_abababababababab", 2, b"ab" * 8, None)):
        spa = K.SynthParams.make(seed=SEED, needle=b"", plant_permille=0, lo=ord("a"), span=span)
        d_a, d_o, d_l, pb = device_arena(None, la, na, spa)
        m.set_patterns([pat])
        m.attach_arena(d_a, d_o, d_l)
        got, _ = m.scan()
        if closed is None:
            m.set_option(OPT_MODE, MODE_AUTOMATON)
            m.set_option(OPT_KERNEL, KERNEL_GENERAL)
            m.attach_arena(d_a, d_o, d_l)
            ref, _ = m.scan()                        # the literal KMP automaton on every byte (kmp_scan_kernel MODE 1)
            m.set_option(OPT_MODE, MODE_FILTER)
            m.set_option(OPT_KERNEL, KERNEL_AUTO)
            m.attach_arena(d_a, d_o, d_l)
            ok, chk = int(got[0]) == int(ref[0]), f"== the KMP-automaton kernel ({int(ref[0])})"
        else:
            ok, chk = int(got[0]) == closed, f"== closed form ({closed})"
        if not ok:
            raise SystemExit(f"extra {name}: count {int(got[0])} fails its check {chk}")
        timed(name, f"{na} x {la} B, text alphabet of {span} letter(s), pattern {pat.decode()!r}: every offset is a candidate", pb, chk)
        del d_a, d_o, d_l
        torch.cuda.empty_cache()
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--settle", type=int, default=400, help="untimed passes before the warm-up so that the GPU's clocks have "
                    "settled (a 250 us kernel needs ~100 ms of load to leave the DVFS transient; profiles/r01_sustained.txt)")
    ap.add_argument("--packets-per-gpu", type=int, default=1_000_000)
    ap.add_argument("--depth", type=int, default=0, help="chunk loads in flight per wavefront (0 = library default)")
    ap.add_argument("--blocks-per-cu", type=int, default=0)
    ap.add_argument("--full", action="store_true", help="after the headline, also time the CPU baseline and the extra_configs legs "
                    "(N = 1); a plain run measures the headline alone")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the per-pattern counts of the last timed step to DIR/counts.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the extra_configs legs (Zipf lengths, strings.txt fused, "
                    "pcap fixture, dense-candidate and adversarial inputs) that follow the timed headline region at N = 1")
    ap.add_argument("--extra-passes", type=int, default=60)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--force-dist", action="store_true", help="rehearsal: create the process group and run the all-reduce path "
                    "even with one rank (checks the RCCL plumbing on a 1-GPU box)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N > 1 (nccl = RCCL; gloo only to rehearse "
                    "the multi-rank code path on a box with fewer GPUs than ranks)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))          # before anything touches the GPU

    import torch
    import torch.distributed as dist

    import multithreading_string_matching_amd as K
    from multithreading_string_matching_amd import dist as kd
    from multithreading_string_matching_amd.matcher import OPT_BLOCKS_PER_CU, OPT_DEPTH, GpuMatcher

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: torch.cuda.is_available() is False (there is no CPU fallback)")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if args.backend == "nccl" else local_rank % max(ndev, 1)
    if dev_index >= ndev:
        raise SystemExit(f"rank {rank}: LOCAL_RANK {local_rank} but only {ndev} GPU(s) visible")
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    n = args.packets_per_gpu
    first_id = rank * n                      # every rank scans its own shard of the global stream
    sp = K.SynthParams.make(seed=SEED, needle=NEEDLE, plant_permille=100)

    # Everything runs on one explicit (non-default) torch stream: the scan kernels are enqueued on it
    # through the C-ABI, and torch.distributed orders its collectives after the CURRENT stream -- so
    # the all-reduce of step i waits for step i's counts and overlaps step i+1's scan.
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    assert stream.cuda_stream != 0
    m = GpuMatcher(dev_index)
    m.set_stream(stream.cuda_stream)
    if args.depth:
        m.set_option(OPT_DEPTH, args.depth)
    if args.blocks_per_cu:
        m.set_option(OPT_BLOCKS_PER_CU, args.blocks_per_cu)

    # ---- synthetic arena, generated on the device ------------------------------------------
    stride = (PAYLOAD_LEN + 15) // 16 * 16
    nbytes = n * stride + 64
    d_arena = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d_arena[n * stride:].zero_()
    d_off = torch.empty(n, dtype=torch.int64, device=dev)
    d_len = torch.empty(n, dtype=torch.int32, device=dev)
    m.fixed_index(d_off, d_len, PAYLOAD_LEN, 16)
    m.synth_fill(d_arena, d_off, d_len, sp, first_pkt_id=first_id)
    m.set_patterns([NEEDLE])
    m.attach_arena(d_arena, d_off, d_len)
    n_chk, payload_bytes = m.arena_info()
    assert (n_chk, payload_bytes) == (n, n * PAYLOAD_LEN)

    # ---- correctness before timing ------------------------------------------------------------
    planted = K.synth_count_planted(sp, n, PAYLOAD_LEN, first_pkt_id=first_id)
    got, _ = m.scan()
    if int(got[0]) != planted:
        raise SystemExit(f"rank {rank}: GPU count {int(got[0])} != planted {planted}")

    # ---- timed region -----------------------------------------------------------------------------
    # The only exchange of the path is the SUM of the per-pattern counters (mpi_dumping.c:202).  Step i leaves
    # its counter in slot i % G of one of two device buffers; a full buffer is all-reduced in ONE collective
    # (G x 8 bytes) while the next G steps fill the other buffer: fewer, larger collectives, none of them on
    # the scan stream's critical path.
    G = 4
    bufs = [torch.zeros(G, dtype=torch.int64, device=dev) for _ in range(2)]
    works = [None, None]

    def step(i):
        b, j = (i // G) % 2, i % G
        if j == 0 and works[b] is not None:
            works[b].wait()                    # this buffer's previous all-reduce has finished (stream-side wait)
            works[b] = None
        m.scan_enqueue(bufs[b][j:j + 1])       # scan kernel + partial reduce -> the slot (device memory)
        if use_dist and j == G - 1:
            works[b] = dist.all_reduce(bufs[b], op=dist.ReduceOp.SUM, async_op=True)

    def drain(n_steps):
        """Reduce the buffer the last steps left partly filled, then wait for everything."""
        if use_dist and n_steps % G:
            b = (n_steps // G) % 2
            works[b] = dist.all_reduce(bufs[b], op=dist.ReduceOp.SUM, async_op=True)
        for b, w in enumerate(works):
            if w is not None:
                w.wait()
                works[b] = None

    for i in range(args.settle):               # device settle-in, not part of W or K
        m.scan_enqueue(bufs[0][0:1])
    torch.cuda.synchronize()
    for i in range(args.warmup):
        step(i)
    drain(args.warmup)
    kd.barrier()
    torch.cuda.synchronize()
    m.profile_begin(args.steps)
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    drain(args.steps)
    torch.cuda.synchronize()
    kd.barrier()
    t1 = time.perf_counter()
    launch_ms = m.profile_end(args.steps)
    elapsed = kd.max_over_ranks(t1 - t0, device=dev)
    avg_launch_ms = kd.max_over_ranks(float(launch_ms.mean()) if len(launch_ms) else 0.0, device=dev)

    last = args.steps - 1
    total = int(bufs[(last // G) % 2][last % G].item())
    planted_all = planted
    if use_dist:
        t = torch.tensor([planted], dtype=torch.int64, device=dev)
        kd.reduce_counts(t)
        planted_all = int(t.item())
    if total != planted_all:
        raise SystemExit(f"rank {rank}: reduced count {total} != planted {planted_all}")
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "counts.npy"), np.array([total], dtype=np.float64))

    # ---- CPU baseline + sample parity (rank 0, N == 1) -------------------------------------------
    cpu = None
    sample97 = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        import oracle
        o = oracle.load()
        host = d_arena.cpu().numpy()
        off = d_off.cpu().numpy().astype(np.uint64)
        ln = d_len.cpu().numpy().astype(np.uint32)
        cores = host_cores()
        best = None
        for _ in range(max(1, args.cpu_reps)):
            counts, dt = o.count(host, off, ln, [NEEDLE], threads=cores)
            if int(counts[0]) != planted:
                raise SystemExit(f"oracle count {int(counts[0])} != GPU/planted {planted}")
            best = dt if best is None else min(best, dt)
        # one-thread figure (the serial.c loop, serial.c:153-155) on the first 100 000 packets
        n1 = min(n, 100_000)
        t1 = time.perf_counter()
        c1, _ = o.count(host, off[:n1], ln[:n1], [NEEDLE], threads=0)
        t1 = time.perf_counter() - t1
        if int(c1[0]) != K.synth_count_planted(sp, n1, PAYLOAD_LEN, first_pkt_id=first_id):
            raise SystemExit("oracle serial count differs from the planted count")
        cpu = {
            "value": round(payload_bytes / best / 1e9, 3), "unit": "GB/s", "cores": cores, "cpu_model": cpu_model(), "kind": "port",
            "serial_1thread_GBps": round(n1 * PAYLOAD_LEN / t1 / 1e9, 3),
            "sample": f"the full per-GPU workload ({n} x {PAYLOAD_LEN} B, 1 pattern), best of {max(1, args.cpu_reps)} passes, "
                      f"openmp_data.c:126-178 bracket, {best:.3f} s per pass",
            "matches_per_s": round(planted / best, 1),
        }
        # Where the reference's own object code travelled with the repo (oracle/_ref, built from /root/reference in the
        # build container): its kmp_matcher (serial.c:190-215), one call per payload, calls spread over the same threads.
        # That is the baseline proper ("reference"); the port's figure stays beside it.
        try:
            ref = oracle.load_ref()
        except Exception:
            ref = None
        if ref is not None and getattr(ref, "has_driver", False):
            rbest = None
            for _ in range(max(1, args.cpu_reps)):
                rc, rdt = ref.count_arena(host, off, ln, NEEDLE, cores)
                if rc != planted:
                    raise SystemExit(f"reference kmp_matcher count {rc} != GPU/planted {planted}")
                rbest = rdt if rbest is None else min(rbest, rdt)
            cpu["port_GBps"] = cpu["value"]
            cpu.update({"value": round(payload_bytes / rbest / 1e9, 3), "kind": "reference",
                        "matches_per_s": round(planted / rbest, 1),
                        "sample": f"the full per-GPU workload ({n} x {PAYLOAD_LEN} B, 1 pattern), best of {max(1, args.cpu_reps)} passes of "
                                  f"the reference's own kmp_matcher object code (serial.c:190-215) over the arena, one call per payload, "
                                  f"{cores} OpenMP threads (guided, as openmp_data.c:157-175), {rbest:.3f} s per pass; the port "
                                  f"(oracle/kmp_oracle.c, openmp_data.c:126-178 bracket) takes {best:.3f} s"})
        # checker for the multi-pattern extra config: the oracle's counts of strings.txt's 97 patterns on the first packets
        if not args.no_extra:
            ns = min(n, 50_000)
            pats97 = K.load_patterns(os.path.join(ROOT, "tests", "golden", "data", "strings.txt"))
            c97, _ = o.count(host, off[:ns], ln[:ns], pats97, threads=cores)
            sample97 = (ns, c97.tolist())
        del host

    # ---- the other BASELINE configs, after the timed headline region (rank 0, N == 1) -----------------
    extra = None
    extra_error = None
    if args.full and rank == 0 and world == 1 and not args.no_extra:
        headline = (d_arena, d_off, d_len, n, PAYLOAD_LEN)
        del d_arena, d_off, d_len
        # a failing leg (a count check included) must not cost the headline line, which has been measured and checked by now:
        # it is reported in the JSON ("extra_configs_error") and on stderr instead
        try:
            extra = extra_configs(m, dev, args.extra_passes, headline, sample97)
        except (SystemExit, Exception) as e:          # noqa: BLE001 -- SystemExit is how the legs report a count mismatch
            extra_error = f"{type(e).__name__}: {e}"
            log(f"extra_configs FAILED: {extra_error}")
        del headline

    if rank == 0:
        bytes_all = payload_bytes * world * args.steps
        value = bytes_all / elapsed / 1e9
        achieved = payload_bytes / (avg_launch_ms * 1e-3) / 1e9 if avg_launch_ms > 0 else 0.0
        # HBM bytes per launch from the PMC counters (FETCH_SIZE x 2 on gfx950, own rocprofv3 pass,
        # profiles/roofline_traffic.json); only valid for the workload it was collected on
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "roofline_traffic.json")
        if os.path.isfile(tpath) and n == 1_000_000:
            with open(tpath) as f:
                traffic = json.load(f).get("hbm_bytes_per_launch")
        out = {
            "metric": "payload GB/s scanned + matches/s, 1M x 1500B pkts, 1 pattern",
            "value": round(value, 2), "unit": "GB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {
                "workload": f"{n} synthetic {PAYLOAD_LEN} B UDP payloads per GPU (a..z, NUL-free, seed {SEED}), "
                            f"one 16-byte pattern planted in ~10% of packets; BASELINE configs[1]",
                "packets_per_gpu": n, "payload_len": PAYLOAD_LEN, "patterns": 1, "pattern_len": len(NEEDLE),
                "parallelism": f"packets sharded over {world} GPU(s), all-reduce(SUM) of counts",
            },
            "rccl_ranks": world if (use_dist and args.backend == "nccl") else 0,
            "backend": (("rccl (torch.distributed nccl)" if args.backend == "nccl" else args.backend) if use_dist else "none (one rank)"),
            "matches_per_s": round(total * args.steps / elapsed, 1),
            "matches_per_pass": total,
            "pct_hbm_peak_per_gpu": round(100.0 * value / world / HBM_PEAK_GBS, 2),
            "roofline": {
                "bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                "traffic_source": (None if traffic is None else "profiles/roofline_traffic.json: FETCH_SIZE x 2 from a separate rocprofv3 --pmc "
                                   "pass over this workload (tools/pmc.sh), a committed constant -- NOT measured by this run"),
                "path": "filter path: the needle's alphabet is disjoint from the text's, candidates only where it was planted (10 % of the "
                        "packets); extra_configs carries the dense-candidate and adversarial figures",
                "kernel": "kmp_scan_flat_kernel", "launch_ms_avg": round(avg_launch_ms, 5),
                "algorithmic_bytes_per_launch": payload_bytes,
            },
            "cpu_baseline": cpu,
            "extra_configs": extra,
            **({"extra_configs_error": extra_error} if extra_error else {}),
        }
        print(json.dumps(out), flush=True)

    m.close()
    if use_dist:
        dist.destroy_process_group()
    if extra_error:
        sys.exit(3)          # the headline line is out; a failed count check of an extra leg still turns the run red


if __name__ == "__main__":
    main()

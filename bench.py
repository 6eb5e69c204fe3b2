"""bench.py — polished reference Mbp/s of the NextPolish2 hot path on MI355X.

Workload = BASELINE.json configs[2]: a S. cerevisiae-sized diploid assembly (17 contigs with the S288C chromosome
lengths, 12.16 Mb), 30x simulated HiFi (15x per haplotype), k21 + k31 yak tables, phasing on (iter_count 2).
A "step" = one pass of the whole hot path (np2_batch_polish: dense diff -> sparse graph -> DP -> LQ regions ->
candidates -> yak scoring -> phasing vote incl. Louvain -> second pass -> seed / recheck / splice) over every contig of
the HBM-resident assembly, polished sequences copied to the host.  The contigs go through the batch driver: one kernel
launch per pipeline step for a group of contigs (csrc/np2_batch.cpp), the way the CLI streams an assembly.
With --gpus N every rank polishes its own assembly (weak scaling, no data-path collective) and the polished sequences
are all-gathered over RCCL inside the timed step.  `--workload ecoli` reproduces the round-1 line (configs[1]).
A plain run sets up, warms up, times --steps steps once and prints the line; --full adds what else the line used to carry
(repeated timed regions, the exclusive roofline steps, host-buffer and files -> FASTA paths, the CPU oracle baseline and
its comparison, the strong sub-result of a multi-rank run).  --dump-outputs DIR writes the last timed step's results.
"""
import argparse
import json
import os
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s peak
# S. cerevisiae S288C: 16 chromosomes + the mitochondrial genome (bp)
YEAST = [230218, 813184, 316620, 1531933, 576874, 270161, 1090940, 562643, 439888, 745751, 666816, 1078177, 924431,
         784333, 1091291, 948066, 85779]
# HBM traffic of one k_diff_reads launch, from rocprofv3 PMC passes (separate --pmc FETCH_SIZE / WRITE_SIZE runs,
# 2 x FETCH_SIZE (gfx950 half-count correction for wide streaming reads) + WRITE_SIZE):
# profiles/r06_yeast_pmc_fetch_write.json (average over the four launches of a step), profiles/r06_ecoli_pmc_fetch_write.json
# (the dense kernel is round 5's: 2 * 26360.4 + 34008.2 and 2 * 38842.8 + 31692.6 KB then; round 4's: 2 * 37805.7 + 38330.9 and 2 * 52134.0 + 38965.5 KB; round 2's: 2 * 31766.7 + 38123.8 and 2 * 48516.1 + 39687.9)
PMC_SOURCE = {"yeast": "profiles/r06_yeast_pmc_fetch_write.json (round 6)", "ecoli": "profiles/r06_ecoli_pmc_fetch_write.json (round 6)"}
# k-mer table probes per polished bp the reference algorithm makes on these workloads (the oracle's kmer_probes stat over
# the whole assembly: kappa of SURVEY.md §8(d)); measured again whenever the cpu_baseline leg runs
KAPPA = {"yeast": 0.66996, "ecoli": 0.38471}
KAPPA_SOURCE = "profiles/r04_kappa.json"
PMC_LAUNCHES = {"yeast": 4, "ecoli": 1}  # launches per step the traffic figure is the per-launch average of
# The roofline kernel is the one that streams the pileup — chosen by BYTES, as the contract's `roofline` asks for the
# dominant kernel of the path's algorithmic traffic — not the one the step spends most time in.  Its share of a step's kernel
# time and the kernel that leads by time, from the tracked one-group kernel tables (rocprofv3 --kernel-trace --stats of
# `bench.py --groups 1`; us per step): not measured in the run that prints the line.
KERNEL_TIME = {"yeast": {"roofline_kernel_us": 145.7, "kernel_sum_us": 3258.5, "dominant_by_time": "k_pf_tile (+ _mid)", "dominant_by_time_us": 583.0,
                         "source": "profiles/r06_yeast_one_group_kernels_per_step.txt (the table's total less k_yak_insert, a context's set-up)"},
               "ecoli": {"roofline_kernel_us": 47.9, "kernel_sum_us": 720.1, "dominant_by_time": "copies of the result to the host (rocclr copyBuffer)", "dominant_by_time_us": 96.2,
                         "source": "profiles/r06_ecoli_kernels_per_step.txt (the table's total less k_yak_insert)"}}
PMC_TRAFFIC = {"yeast": int((2 * 26312.2 + 33996.6) * 1024), "ecoli": int((2 * 38836.5 + 31654.1) * 1024)}
DUMP_BYTES = 64 << 20  # budget of --dump-outputs over all its files


def dump_outputs(d, bases, spans, budget=DUMP_BYTES):
    """--dump-outputs: what a caller of the timed path receives from its last step, as .npy files in d —
    polished_bases.npy (float32 of the bases' ASCII codes, every contig's one after the other), contig_lengths.npy and
    spans.npy (float64; first and last reference position per contig).  Bases beyond the budget: a fixed sample (seed 0)
    of them, polished_bases_index.npy (float64) saying which."""
    os.makedirs(d, exist_ok=True)
    lengths = np.array([len(b) for b in bases], dtype=np.float64)
    spans = np.array([[int(x[0]), int(x[1])] for x in spans], dtype=np.float64).reshape(-1, 2)
    flat = np.concatenate([np.asarray(b).view(np.uint8).ravel() for b in bases]) if bases else np.zeros(0, np.uint8)
    room = budget - lengths.nbytes - spans.nbytes - 4 * 128  # (.npy headers)
    index = None
    if flat.size * 4 > room:  # a sampled base costs 4 B of value + 8 B of index
        index = np.unique(np.random.default_rng(0).integers(0, flat.size, size=room // 12))
        flat = flat[index]
    np.save(os.path.join(d, "polished_bases.npy"), flat.astype(np.float32))
    np.save(os.path.join(d, "contig_lengths.npy"), lengths)
    np.save(os.path.join(d, "spans.npy"), spans)
    if index is not None:
        np.save(os.path.join(d, "polished_bases_index.npy"), index.astype(np.float64))


def make_assembly(lengths, depth, seed0, diploid):
    from nextpolish2_amd.synth import Synth
    def one(a):
        kw = {}
        if os.environ.get("NP2_BENCH_ERR_SCALE"):  # experiments only: error rates of the generator scaled (0 = none)
            f = float(os.environ["NP2_BENCH_ERR_SCALE"])
            kw = dict(read_err_rate=0.002 * f, asm_err_rate=1e-4 * f, snp_rate=0.005 * f, hap_indel_rate=0.002 * f)
        s = Synth(a[1], depth=depth, seed=seed0 + a[0], diploid=diploid, name=f"chr{a[0] + 1}", **kw)
        # reads in coordinate order (ties in generation order), the order a sorted BAM presents them in: the resident
        # pileups and the BAM written from the same generator (Synth.bam_records) then describe the same input
        r = s.pileup.reads
        r[1:] = r[1:][np.argsort(r["aln_t_s"][1:], kind="stable")]
        return s
    with ThreadPoolExecutor(min(16, len(lengths))) as ex:  # (the generator runs outside the GIL)
        return list(ex.map(one, enumerate(lengths)))


class Groups:
    """The assembly's contigs split over G batch groups of about equal size in bp (longest contig first, each to the
    least loaded group): each group is one
    np2_batch_t driven by its own host thread, so one group's host phases (the Louvain of the phasing vote, ~1 ms for
    the longest contig) and read-back latencies are filled by the other groups' kernels.  Over the K timed steps the
    groups run free — every group polishes its contigs K times, the groups do not wait for each other between steps
    (a step's output is complete when the slowest group has delivered it) — the way a server works through a queue of
    assemblies.  Stream priorities alternate high / low over the groups: equal-priority streams advance in lockstep
    and meet in their host phases."""

    def __init__(self, pol, contigs, lengths, n_groups):
        from nextpolish2_amd import BatchPolisher
        order = sorted(range(len(contigs)), key=lambda i: -lengths[i])
        # longest contig first, each to the group with the least bp so far: the groups run free over the steps, so the
        # job ends with the slowest group (cut into equal shares in input order the last group got 1.3 of 12 Mb)
        n_groups = max(1, min(n_groups, len(order)))
        self.members, load = [[] for _ in range(n_groups)], [0] * n_groups
        for i in order:
            g = min(range(n_groups), key=lambda j: (load[j], j))
            self.members[g].append(i)
            load[g] += lengths[i]
        self.bps = [BatchPolisher(pol, len(m)) for m in self.members]
        if len(self.bps) > 1:
            for g, b in enumerate(self.bps):
                b.set_priority(g % 2 == 0)
        self.contigs = contigs
        self.n = len(contigs)
        # how many steps the groups may run in front of the per-step collective of a multi-rank run (one staging buffer each)
        self.ahead = max(1, int(os.environ.get("NP2_BENCH_GATHER_AHEAD", "1")))

    def set_timing(self, on):
        for b in self.bps:
            b.set_timing(on)

    def slot_results(self, g):
        """[(contig index, device address, length)] of group g's last wave (np2_last_result_device of its slot contexts)."""
        import ctypes as C
        from nextpolish2_amd.api import lib
        out = []
        for slot, i in enumerate(self.members[g]):
            p, n = C.c_void_p(), C.c_uint64()
            rc = lib().np2_last_result_device(lib().np2_batch_slot_ctx(self.bps[g]._h, slot), C.byref(p), C.byref(n))
            if rc != 0:
                raise RuntimeError("np2_last_result_device on a batch slot")
            out.append((i, p.value, n.value))
        return out

    def run(self, opts, steps, after_step=None, exclusive=False, stage=None, sink=None):
        """`steps` passes over the assembly.  after_step(out) runs on the calling thread once every group has delivered
        a step (the groups may be one step ahead of it by then).  stage(k, items): called on a group's thread when it has
        delivered step k, with slot_results of its contigs (the multi-rank run copies them, device to device, into the
        buffer the step's all-gather sends).  sink(k, i) -> (device address, capacity): instead of `stage`, the batch driver
        itself copies contig i's polished bases of step k there (np2_batch_set_sink).  exclusive: one group at a time (the roofline kernel
        measured without other kernels next to it).  -> (outputs of the last step, per-step sum of the k_diff_reads
        launch durations in ms, launches per step, mean np2_batch_polish call time in ms)"""
        G = len(self.bps)
        NB = self.ahead + 1  # steps whose outputs may be pending at once (the groups run up to `ahead` steps in front of after_step)
        outs = [[None] * self.n for _ in range(NB)]
        done, seen = [0] * G, [0]
        acc = [[0.0, 0, 0.0, 0.0, 0.0, 0.0] for _ in range(G)]
        cv = threading.Condition()
        turn = [0]

        def loop(g):
            for k in range(steps):
                with cv:
                    cv.wait_for(lambda: (after_step is None or seen[0] >= k - self.ahead) and (not exclusive or turn[0] % G == g))
                if sink is not None:  # where this step's polished bases go on the device (the buffer the step's all-gather sends)
                    for slot, i in enumerate(self.members[g]):
                        self.bps[g].set_sink(slot, *sink(k, i))
                res = self.bps[g].polish([self.contigs[i] for i in self.members[g]], opts)
                for i, r in zip(self.members[g], res):
                    outs[k % NB][i] = r
                if stage is not None:
                    stage(k, self.slot_results(g))
                ms, launches = self.bps[g].last_diff_ms()
                acc[g][0] += ms
                acc[g][1] = launches
                acc[g][2] += self.bps[g].last_call_ms
                inside, tail = self.bps[g].last_call_ms_inside()
                acc[g][3] += inside
                acc[g][4] += tail
                acc[g][5] += self.bps[g].flush_total_ms()
                with cv:
                    done[g] = k + 1
                    turn[0] += 1
                    cv.notify_all()
        ths = [threading.Thread(target=loop, args=(g,)) for g in range(G)]
        for t in ths:
            t.start()
        if after_step is not None:
            for k in range(steps):
                with cv:
                    cv.wait_for(lambda: min(done) >= k + 1)
                after_step(outs[k % NB]) if (stage is None and sink is None) else after_step(k, outs[k % NB])
                with cv:
                    seen[0] = k + 1
                    cv.notify_all()
        for t in ths:
            t.join()
        self.call_breakdown = {  # per group, mean over the steps, ms: the caller's clock around the C call, the call's own
            # clock, the flushes inside it (host phase + issue + wait) and what follows the last flush
            "caller_clock": [round(x[2] / max(1, steps), 3) for x in acc], "inside_call": [round(x[3] / max(1, steps), 3) for x in acc],
            "flushes": [round(x[5] / max(1, steps), 3) for x in acc], "after_last_flush": [round(x[4] / max(1, steps), 3) for x in acc]}
        return (outs[(steps - 1) % NB], sum(x[0] for x in acc) / max(1, steps), sum(x[1] for x in acc),
                sum(x[2] for x in acc) / max(1, steps * G))


def thread_cpu_ns():
    """run time in ns of every thread of this process so far (schedstat), with its name"""
    out = {}
    for tid in os.listdir("/proc/self/task"):
        try:
            ns = int(open(f"/proc/self/task/{tid}/schedstat").read().split()[0])
            out[int(tid)] = (ns, open(f"/proc/self/task/{tid}/comm").read().strip())
        except Exception:
            pass
    return out


def cpu_throttle_stat():
    """(periods, throttled periods, throttled microseconds) of this container's CPU quota so far (cgroup v2), or None"""
    try:
        d = dict(l.split() for l in open("/sys/fs/cgroup/cpu.stat"))
        return int(d.get("nr_periods", 0)), int(d.get("nr_throttled", 0)), int(d.get("throttled_usec", 0))
    except Exception:
        return None


def cpu_baseline(syn, yaks, opts, max_threads, n_jobs=256):
    """The CPU oracle run like the reference: one contig per worker thread (main.rs:1717-1843), ONE in-memory copy of the
    k-mer tables shared by the workers, as many workers as this process may use CPUs — the cgroup quota, not the number
    of hardware threads the box shows (nextpolish2_amd/_cpus.py: on the GPU boxes 16 of 256; beyond the quota threads are
    only throttled: profiles/r03_cpu_baseline_scaling_probe.log) — each pulling contigs off one queue of `n_jobs` (the
    assembly's 17, replicated, so that every worker has real work to the end)."""
    from nextpolish2_amd._cpus import usable_cpus
    from oracle.np2_oracle import Oracle
    cores = os.cpu_count() or 1
    usable = usable_cpus()
    n_thr = max(1, min(max_threads or usable, usable))
    base = Oracle(yaks)
    # single-thread rate first (largest contig).  The first polish also builds the shared tables (filtered for
    # min_kmer_count, sorted per bucket) before the workers clone the oracle: it is NOT timed (16 x the
    # single-thread figure did not match the 16-thread one because the table build was inside it) — the second one is
    big = max(range(len(syn)), key=lambda i: syn[i].pileup.L)
    t0 = time.perf_counter()
    base.polish(syn[big].pileup, opts)
    t1 = time.perf_counter()
    ob, op = base.polish(syn[big].pileup, opts)
    st = time.perf_counter() - t1
    single = syn[big].pileup.L / st / 1e6
    tables_s = max(0.0, (t1 - t0) - st)
    results, probes = {}, {}

    def run(n, jobs_wanted):
        # n worker threads pull contigs from one queue (the reference's bounded channel, main.rs:1700-1715)
        jobs = [i % len(syn) for i in range(max(n, jobs_wanted, len(syn)))]
        nxt = [0]
        lock = threading.Lock()
        done = [0] * n

        def work(w):
            orc = base.clone(opts.min_kmer_count)
            while True:
                with lock:
                    j = nxt[0]
                    nxt[0] += 1
                if j >= len(jobs):
                    return
                r = orc.polish(syn[jobs[j]].pileup, opts)
                done[w] += syn[jobs[j]].pileup.L
                if j < len(syn):
                    results[jobs[j]] = r
                    probes[jobs[j]] = orc.stats()["kmer_probes"]  # k-mer table probes the reference algorithm makes
        ths = [threading.Thread(target=work, args=(w,)) for w in range(n)]
        t1 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t1
        return sum(done) / dt / 1e6, dt, len(jobs)

    v_all, dt_all, jobs_all = run(n_thr, n_jobs)
    # variant (i) of BASELINE.md §3: what a user of the reference experiences — no table in memory, every scoring phase
    # of every contig (1 + 1 + n_yak per contig) re-streams the .yak dumps from disk (kmer.rs:132-170)
    import tempfile
    from nextpolish2_amd import io as np2io
    with tempfile.TemporaryDirectory() as td:
        paths = []
        for y in yaks:
            paths.append(os.path.join(td, f"k{y.k}.yak"))
            np2io.write_yak(paths[-1], y)
        base.set_yak_files(paths)
        v_stream, dt_stream, jobs_stream = run(n_thr, len(syn))
        base.set_yak_files(None)
    return {"value": round(v_all, 4), "unit": "Mbp/s", "cores": n_thr, "kind": "port",
            "yak_restreaming": {"value": round(v_stream, 4), "unit": "Mbp/s", "cores": n_thr, "wall_s": round(dt_stream, 1),
                                "what": "variant (i): each scoring phase re-reads the .yak dumps (8 KiB buffered reads, one "
                                        "hash-set probe per file word) like KmerInfo::retrieve_kmers; same results; one pass "
                                        f"over the assembly's {jobs_stream} contigs"},
            "sample": f"{jobs_all} contigs (the assembly's {len(syn)}, replicated) through one queue on {n_thr} worker threads, one "
                      f"contig per thread like the reference's workers (main.rs:1717-1843), in-memory k-mer tables, one "
                      f"shared copy (variant (ii) of BASELINE.md): {v_all:.2f} Mbp/s in {dt_all:.1f} s",
            "single_thread": round(single, 4), "single_thread_what": "largest contig, second polish of the context (tables built by the first)",
            "tables_build_s": round(tables_s, 2), "host_cores": cores, "usable_cpus": usable,
            "kmer_probes_per_bp": round(sum(probes.values()) / max(1, sum(syn[i].pileup.L for i in probes)), 5),
            "note": "usable_cpus = the container's CFS quota (cpu.max); the box shows host_cores hardware threads, but threads "
                    "beyond the quota are throttled, not run (profiles/r03_cpu_baseline_scaling_probe.log: 256 threads reach "
                    "a third of the 17-thread rate with 238 s of system time)"}, results


def kernel_path_host_buffers(pol, syn, opts, bases, workers=4):
    """SURVEY.md §8(d)'s kernel-path definition, literally: the packed pileups sit in HOST memory (pageable numpy arrays,
    as an FFI caller would hold them) and every contig goes through np2_polish_contig = upload (H2D of the nibble
    streams, descriptors, tile read lists) + polish + free; `workers` contexts share the k-mer tables and keep that
    many contigs in flight.  The headline `value` starts from HBM-resident pileups instead."""
    ctxs = [pol] + [pol.clone() for _ in range(workers - 1)]
    order = sorted(range(len(syn)), key=lambda i: -syn[i].pileup.L)
    best, same = None, True
    for rep in range(3):
        out = [None] * len(syn)
        nxt, lock = [0], threading.Lock()

        def work(w):
            while True:
                with lock:
                    j = nxt[0]
                    nxt[0] += 1
                if j >= len(order):
                    return
                i = order[j]
                c = ctxs[w].upload(syn[i].pileup)
                try:
                    out[i] = ctxs[w].polish_resident(c, opts, want_pos=False)[0]
                finally:
                    c.free()
        t0 = time.perf_counter()
        ths = [threading.Thread(target=work, args=(w,)) for w in range(workers)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
        same = same and all(np.array_equal(out[i], bases[i]) for i in range(len(syn)))
    total = sum(s.pileup.L for s in syn)
    nbytes = sum(int(s.pileup.nibbles.shape[0]) for s in syn)
    per_contig = {"value": round(total / best / 1e6, 2), "unit": "Mbp/s", "wall_ms": round(best * 1e3, 2), "workers": workers,
                  "h2d_gbs_at_least": round(nbytes / best / 1e9, 2), "identical_to_resident_path": bool(same),
                  "path": "np2_polish_contig (upload + polish + free) per contig, one after the other on each of "
                          f"{workers} contexts sharing the k-mer tables: launch-bound plain contexts; best of 3"}
    # The same host buffers through the batch driver, the way the headline's resident pileups are polished: every group's
    # thread uploads its own contigs (np2_contig_upload on a context of its own: the copies of the groups share the link)
    # and hands them to its np2_batch_t; the clock stops when every polished sequence is on the host.  A link that moves a
    # pageable buffer at 56 GB/s (tools/ubench_h2d.hip) carries the assembly's 186 MB in 3.3 ms.
    lengths = [s.pileup.L for s in syn]
    grp = Groups(pol, [None] * len(syn), lengths, workers)
    best_b, same_b = None, True
    for rep in range(3):
        out = [None] * len(syn)
        held = [[] for _ in grp.members]

        def work_b(g):
            cs = [ctxs[g % len(ctxs)].upload(syn[i].pileup) for i in grp.members[g]]
            held[g] = cs
            for i, r in zip(grp.members[g], grp.bps[g].polish(cs, opts)):
                out[i] = r[0] if isinstance(r, tuple) else r
        t0 = time.perf_counter()
        ths = [threading.Thread(target=work_b, args=(g,)) for g in range(len(grp.members))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
        best_b = dt if best_b is None else min(best_b, dt)
        same_b = same_b and all(np.array_equal(out[i], bases[i]) for i in range(len(syn)))
        for cs in held:
            for c in cs:
                c.free()
    for b in grp.bps:
        b.close()
    for c in ctxs[1:]:
        c.close()
    return {"value": round(total / best_b / 1e6, 2), "unit": "Mbp/s", "wall_ms": round(best_b * 1e3, 2), "groups": len(grp.members),
            "h2d_bytes": nbytes, "h2d_gbs_at_least": round(nbytes / best_b / 1e9, 2),  # (the polish itself is inside the same wall time)
            "identical_to_resident_path": bool(same_b),
            "path": "host-resident packed pileups -> np2_contig_upload of a group's contigs on the group's own thread -> "
                    "np2_batch_polish of the group -> polished sequences on the host; the groups side by side; best of 3",
            "per_contig_call": per_contig}


def end_to_end(pol, syn_c, yaks, opts, tmpdir, resident_result):
    """BAM + FASTA + yak files -> polished FASTA record for ONE contig through np2_contig_from_bam (BGZF inflate, record
    parse, H2D, GPU columnariser, polish, D2H): the rate a drop-in user of the CLI sees per contig."""
    from nextpolish2_amd import io as np2io
    from nextpolish2_amd.bamio import pileup_to_records, write_bam
    recs = pileup_to_records(syn_c.pileup, decorate=False)
    bam_path = os.path.join(tmpdir, "e2e.bam")
    write_bam(bam_path, [(syn_c.pileup.name, syn_c.pileup.L)], recs)
    ref = syn_c.pileup.ref.tobytes()
    bam = np2io.Bam(bam_path)
    best = None
    for _ in range(5):  # (the first call pays thread-pool start and first-touch of the staging buffers)
        t0 = time.perf_counter()
        c = np2io.contig_from_bam(pol, bam, syn_c.pileup.name, ref)
        t1 = time.perf_counter()
        b, span = pol.polish_resident(c, opts, want_pos=False)
        rec = b">%s start:%d end:%d\n%s\n" % (syn_c.pileup.name.encode(), span[0], span[1], b.tobytes())
        t2 = time.perf_counter()
        c.free()
        if best is None or t2 - t0 < best[0]:
            best = (t2 - t0, t1 - t0, t2 - t1)
    # the same contig with its reads extracted ON THE DEVICE (NP2_INFLATE=gpu: BGZF blocks uploaded as they lie in the file,
    # inflated one wavefront per block, records walked along the .bai linear index, SEQ read in place): what a rank with a
    # share of two host CPUs would run by default; here on all of this process's CPUs, next to the host pool's figure above
    dev = None
    old_mode = os.environ.get("NP2_INFLATE")
    try:
        os.environ["NP2_INFLATE"] = "gpu"
        bd = None
        for _ in range(4):
            t0 = time.perf_counter()
            c = np2io.contig_from_bam(pol, bam, syn_c.pileup.name, ref)
            t1 = time.perf_counter()
            b2, _sp = pol.polish_resident(c, opts, want_pos=False)
            c.free()
            if bd is None or t1 - t0 < bd:
                bd = t1 - t0
        data = np.fromfile(bam_path, dtype=np.uint8)
        infl, k_ms = np2io.bgzf_inflate_device(pol, data)
        infl, k_ms = np2io.bgzf_inflate_device(pol, data)
        dev = {"front_end_ms": round(bd * 1e3, 2), "identical_to_resident_path": bool(np.array_equal(b2, resident_result)),
               "inflate_kernel_ms": round(k_ms, 3), "inflated_bytes": int(len(infl)),
               "inflate_gbs": round(len(infl) / max(k_ms, 1e-6) / 1e6, 2),
               "note": "k_bgzf_inflate over the whole file (HIP events); the host pool's front end is front_end_ms above"}
    except Exception as e:  # (reported, not fatal: the host path above is the default at this CPU count)
        dev = {"error": str(e)[:200]}
    finally:
        if old_mode is None:
            os.environ.pop("NP2_INFLATE", None)
        else:
            os.environ["NP2_INFLATE"] = old_mode
    return {"value": round(syn_c.pileup.L / best[0] / 1e6, 2), "unit": "Mbp/s", "contig_bp": syn_c.pileup.L,
            "front_end_ms": round(best[1] * 1e3, 2), "polish_ms": round(best[2] * 1e3, 2),
            "bam_bytes": os.path.getsize(bam_path), "identical_to_resident_path": bool(np.array_equal(b, resident_result)),
            "read_extraction_on_device": dev,
            "path": "BAM (BGZF) -> np2_contig_from_bam -> np2_polish_resident -> FASTA record, one contig, one context"}


def end_to_end_assembly(syn, yaks, tmpdir, bases, spans, workers=2):
    """The whole assembly through the command line's own code path (nextpolish2_amd.cli.main, in process): yak dumps,
    FASTA and one coordinate-sorted indexed BAM on local disk -> polished FASTA file.  The wall time includes loading
    the yak files and building the HBM tables; `workers` contexts keep that many contigs in flight (front end of one
    contig next to the kernels of the others)."""
    from nextpolish2_amd import cli
    from nextpolish2_amd import io as np2io
    from nextpolish2_amd.bamio import write_bam_raw
    refs = [(s.pileup.name, s.pileup.L) for s in syn]
    bam = os.path.join(tmpdir, "asm.bam")
    write_bam_raw(bam, refs, [s.bam_records(i) for i, s in enumerate(syn)])
    fa = os.path.join(tmpdir, "asm.fa")
    with open(fa, "wb") as f:
        for s in syn:
            f.write(b">%s\n%s\n" % (s.pileup.name.encode(), s.pileup.ref.tobytes()))
    yk = []
    for y in yaks:
        yk.append(os.path.join(tmpdir, f"k{y.k}.yak"))
        np2io.write_yak(yk[-1], y)
    walls, b2b = [], []
    for rep in range(7):
        out = os.path.join(tmpdir, f"out{rep}.fa")
        # Runs 0-3 each start 0.25 s after the one before: a run burns ~1.1 CPU-seconds in ~45 ms (the host pool inflates the
        # assembly's 600 MB on every hardware thread), and in a container with a CFS quota (16 CPUs here: 1.6 CPU-seconds per
        # 100 ms period) a run that starts in the period the previous one exhausted has all its threads stopped for the rest
        # of it, 30-45 ms at a stretch.  The pause is outside the timed region.  Runs 4-6 follow each
        # other at once: what the quota sustains (`back_to_back`).
        if 0 < rep <= 4:
            time.sleep(0.25)
        t0 = time.perf_counter()
        rc = cli.main([bam, fa] + yk + ["-o", out, "-t", str(workers), "-L", "20000"])  # (default -L 1000000 passes short contigs through)
        (walls if rep < 4 else b2b).append(time.perf_counter() - t0)
        if rc != 0:
            raise RuntimeError("cli.main failed")
    best = min(walls)
    want = b"".join(b">%s start:%d end:%d\n%s\n" % (s.pileup.name.encode(), spans[i][0], spans[i][1], bases[i].tobytes())
                    for i, s in enumerate(syn))
    total = sum(s.pileup.L for s in syn)
    return {"value": round(total / best / 1e6, 2), "unit": "Mbp/s", "wall_s": round(best, 3), "assembly_bp": total,
            "first_run": {"value": round(total / walls[0] / 1e6, 2), "wall_s": round(walls[0], 3)},
            "all_runs_wall_s": [round(w, 3) for w in walls],
            "back_to_back": {"value": round(total * len(b2b) / sum(b2b) / 1e6, 2), "unit": "Mbp/s", "runs_wall_s": [round(w, 3) for w in b2b],
                             "note": "three runs one right after the other: the rate the container's CPU quota sustains"},
            "bam_bytes": os.path.getsize(bam), "yak_bytes": sum(os.path.getsize(p) for p in yk), "workers": workers,
            "identical_to_resident_path": open(out, "rb").read() == want,
            "path": "k21/k31 .yak + FASTA + BAM (BGZF, .bai) files -> nextPolish2 command line (in process; reading the dumps "
                    "and building the HBM tables included: ~10-20 ms, streamed to the device while the first alignments "
                    "are read) -> FASTA file; value = best of 4 runs started 0.25 s apart, first_run = the first one: every run makes and "
                    "releases its own contexts, tables and BAM handles, but from the second on their streams, pinned "
                    "staging and device blocks come from the process-wide pools the first run filled"}


def dist_setup():
    """(rank, world, device index, torch device of this rank's GPU, device the collectives' tensors live on, backend).
    NP2_BENCH_BACKEND (default nccl = RCCL over xGMI) picks the torch.distributed backend: with gloo the collectives go
    through host memory, which lets several ranks share ONE GPU — the rehearsal of the multi-rank code paths on a
    one-GPU box (tests/test_gpu_dist.py); a rank's device is LOCAL_RANK modulo the devices the box has."""
    import torch
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    backend = os.environ.get("NP2_BENCH_BACKEND", "nccl")
    idx = local_rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(idx)
    dev = torch.device("cuda", idx)
    from nextpolish2_amd.dist import note_ranks_per_device
    note_ranks_per_device(int(os.environ.get("LOCAL_WORLD_SIZE", world)), torch.cuda.device_count())
    if "RANK" in os.environ:  # launched by torch.distributed.run (also with one rank: same code path)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)
    cdev = dev if backend == "nccl" else torch.device("cpu")
    return rank, world, idx, dev, cdev, backend


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: re-run this command line under torch.distributed.run with N ranks on
    this node (127.0.0.1 rendezvous on a free port) and relay their output; rank 0's JSON line carries n_gpus == N."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE)
    out = p.stdout.decode(errors="replace")
    sys.stdout.write(out)
    sys.stdout.flush()
    lines = [json.loads(x) for x in out.splitlines() if x.startswith("{")]
    if p.returncode != 0 or not lines or lines[-1].get("n_gpus") != n:
        raise SystemExit(f"bench.py --gpus {n}: the ranks did not deliver a line with n_gpus == {n} (exit code {p.returncode})")
    return 0


def main_strong(a):
    """`--scaling strong`: the strong-scaling line on its own (strong_measure below) — BASELINE configs[3], ONE contig of
    248 Mb by default, diploid ("chr1 with injected SNV / indel") unless --haploid."""
    setup = dist_setup()
    if setup[1] != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={setup[1]}")
    import torch.distributed as dist
    out_line = strong_measure(a, setup, a.contig_mb * a.scale, a.steps, a.warmup, not a.haploid,
                              cpu_base=a.full and not a.no_cpu_baseline, dump=a.dump_outputs)
    if setup[0] == 0:
        print(json.dumps(out_line), flush=True)
    if "RANK" in os.environ:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def strong_measure(a, setup, contig_mb, steps, warmup, diploid, cpu_base=False, dump=None):
    """Strong scaling: ONE contig, 30x simulated HiFi (15x per haplotype when diploid), k21 + k31, cut into one reference
    interval per rank (np2_shard_*; nextpolish2_amd.dist.polish_sharded).  The shards are resident in HBM before the timed
    region; a step = the whole hot path of the contig: every rank's dense pass, its phasing pass, the votes gathered onto
    rank 0 (RCCL), the contig-wide decision there, the removed reads broadcast, the final pass, the strips around the cuts
    exchanged and checked, the owned slices gathered from the device buffers onto rank 0 (RCCL over xGMI) and landed in one
    host array there.  dump: directory for dump_outputs of the last timed step (rank 0).  Returns the JSON object of the
    line (complete on rank 0)."""
    import torch
    import torch.distributed as dist
    from nextpolish2_amd import Opts, Polisher
    from nextpolish2_amd.api import free_shard, shard_plan, upload_shard
    from nextpolish2_amd.dist import polish_sharded
    from nextpolish2_amd.synth import Synth, concat_pileups

    rank, world, local_rank, dev, cdev, backend = setup
    distributed = "RANK" in os.environ
    L = int(contig_mb * 1e6)
    n_parts = 16
    # every rank generates the same contig (seeded) and keeps only its shard in HBM
    with ThreadPoolExecutor(min(n_parts, os.cpu_count() or 1)) as ex:
        parts = list(ex.map(lambda i: Synth(L // n_parts, depth=a.depth, seed=500 + i, diploid=diploid), range(n_parts)))
    pu = concat_pileups([p.pileup for p in parts], "chr1")
    ks = [21, 31]
    yaks = [Synth.yak_assembly(parts, k) for k in ks]
    truth = b"".join(p.hap1 for p in parts)
    del parts
    pol = Polisher(yaks, device=local_rank)
    plans = shard_plan(pu, world, 65536)
    shard = upload_shard(pol, pu, plans[rank])
    opts = Opts()
    last = [None]

    def step():
        b, _, span = polish_sharded(pol, pu, opts, device=cdev if distributed else None, want_pos=False, dst=0, with_span=True,
                                    plans=plans, resident=shard)
        last[0] = (b, span)

    def sync():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    diff_ms = []
    for _ in range(warmup):
        step()
    import gc
    gc.collect()
    gc.disable()
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
        tm = pol.timings()
        diff_ms.append(tm.get("diff_reads", 0.0))  # HIP events around k_diff_reads on the context's own stream
        if "diff_probe" in tm:  # (NP2_DENSE_PROBE: a part of the dense pass launched once more, tools/dense_probe.sh)
            print(f"diff_probe {tm['diff_probe']:.4f} ms (diff_reads {tm.get('diff_reads', 0.0):.4f})", file=sys.stderr)
    sync()
    dt = time.perf_counter() - t0
    gc.enable()
    if dump and rank == 0:
        dump_outputs(dump, [last[0][0]], [last[0][1]])
    stages = None
    if os.environ.get("NP2_BENCH_STAGES"):  # one more, untimed step with every stage timer armed: where a step's time goes
        pol.set_timing(True)
        step()
        stages = {k: round(v, 3) for k, v in sorted(pol.timings().items(), key=lambda kv: -kv[1])}
        pol.set_timing(False)
        os.environ["NP2_DIST_PROFILE"] = "1"  # ... and the wall clock of the protocol's phases on this rank (Python side included)
        t1 = time.perf_counter()
        step()
        from nextpolish2_amd.dist import PHASE_MS
        stages = {"protocol_phases_ms": {k: round(v, 2) for k, v in PHASE_MS.items()}, "protocol_step_ms": round((time.perf_counter() - t1) * 1e3, 2),
                  "context_stage_ms": stages}
        del os.environ["NP2_DIST_PROFILE"]
    if distributed:
        t = torch.tensor([dt], dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    value = pu.L * steps / dt / 1e6
    # roofline of this rank's k_diff_reads launch: the reads of its zone, whole (sub-contig [sub_lo, sub_hi))
    pl = plans[rank]
    rd = pu.reads[pl.read_lo:pl.read_hi]
    inz = (rd["aln_t_e"] >= pl.zone_lo) & (rd["aln_t_s"] < pl.zone_hi) & ((rd["flags"] & 1) == 0)
    cols = int(rd["n_cols"][inz].astype(np.int64).sum())
    alg_bytes = 0.5 * cols + 0.5 * (pl.sub_hi - pl.sub_lo)
    avg_ms = float(np.mean(diff_ms)) if diff_ms else 0.0
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    out_line = {
        "metric": "polished reference Mbp/s (whole node) at 30x HiFi + k21/k31; FASTA identical to oracle",
        "value": round(value, 3), "unit": "Mbp/s", "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": round(dt / steps * 1e3, 3), "higher_is_better": True, "scaling": "strong",
        "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": f"one {'diploid' if diploid else 'haploid'} contig of {pu.L / 1e6:.1f} Mb (BASELINE configs[3]: human chr1 is 248 Mb), "
                               f"30x simulated HiFi{' (15x per haplotype)' if diploid else ''}, "
                               f"k21 + k31 yak, cut into {world} reference interval(s), one per MI355X",
                   "diploid": bool(diploid),
                   "contig_bp": pu.L, "depth": a.depth, "reads": pu.n_reads, "pileup_columns": int(pu.n_columns()) - pu.L,
                   "yak_k": ks, "iter_count": 2, "halo": 65536, "verify": 1024,
                   "parallelism": f"reference-interval shards x{world}: votes all-gathered and decided contig-wide per phasing "
                                  f"pass, owned slices gathered from the device buffers onto rank 0",
                   "output": "the polished contig in one host array on rank 0 inside the step"},
        "roofline": {"bound": "hbm", "kernel": "k_diff_reads", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": None,
                     "alg_bytes_per_launch": int(alg_bytes), "launches_per_step": 1, "avg_launch_ms": round(avg_ms, 4),
                     "units_per_launch_bp": int(pl.sub_hi - pl.sub_lo), "note": "rank 0's launch over its shard"},
    }
    if stages is not None:
        out_line["stage_ms_one_step"] = stages
    if rank == 0:
        b, span = last[0]
        if not diploid:  # (a diploid contig is polished towards its reads' haplotypes: no single truth string)
            out_line["polished_equals_truth"] = bool(b.tobytes() == truth)
        import zlib
        out_line["output_crc32"] = zlib.crc32(b.tobytes())  # (the same contig whatever N: the N-rank result must reproduce it)
        out_line["span"] = [int(span[0]), int(span[1])]
    if rank == 0 and world == 1 and cpu_base:
        # CPU baseline on a bounded sample: the reference polishes one contig on ONE thread whatever -t says
        # (main.rs:1726-1837), so the sample is a shorter contig of the same recipe on one core
        from oracle.np2_oracle import Oracle
        sm = Synth(8_000_000, depth=a.depth, seed=77, diploid=diploid)
        ys = [sm.yak(k) for k in ks]
        t1 = time.perf_counter()
        ob, op = Oracle(ys).polish(sm.pileup, opts)
        st = time.perf_counter() - t1
        g = Polisher(ys, device=local_rank)
        gb, gp = g.polish(sm.pileup, opts)
        out_line["cpu_baseline"] = {"value": round(sm.pileup.L / st / 1e6, 4), "unit": "Mbp/s", "cores": 1, "kind": "port",
                                    "sample": "an 8 Mb contig of the same recipe on one host thread: the reference gives a contig "
                                              "to ONE worker thread (main.rs:1726-1837), a one-contig input runs on one core "
                                              "whatever -t says",
                                    "wall_s": round(st, 1)}
        out_line["fasta_identical_to_oracle"] = bool(np.array_equal(ob, gb) and np.array_equal(op, gp))
    free_shard(pol, shard)
    return out_line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", choices=["yeast", "ecoli", "chr1"], default="yeast")
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--scale", type=float, default=1.0, help="scale every contig length (tests; the metric is quoted at 1.0)")
    ap.add_argument("--groups", type=int, default=4, help="batch groups (host threads driving one np2_batch_t each)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-end-to-end", action="store_true")
    ap.add_argument("--no-exclusive", action="store_true", help="skip the two untimed steps behind roofline_exclusive (profiling runs)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="host threads of the CPU baseline (0 = all cores)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak (default): one assembly per GPU (BASELINE configs[2] at N = 1); strong: ONE long contig "
                         "(--workload chr1, BASELINE configs[3]) cut into one reference interval per GPU")
    ap.add_argument("--contig-mb", type=float, default=248.0, help="--scaling strong: length of the contig in Mb")
    ap.add_argument("--haploid", action="store_true", help="--scaling strong: a haploid contig (no phasing vote to decide)")
    ap.add_argument("--strong-mb", type=float, default=62.0,
                    help="--gpus N > 1: length of the diploid contig behind the 'strong' sub-result of the weak line (0: none)")
    ap.add_argument("--repeats", type=int, default=None,
                    help="timed regions of --steps steps each: the first is the line's value, all of them its median / min / max "
                         "(default 5 with --full, else 1)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: repeated timed regions, the exclusive "
                         "roofline steps, host-buffer and files -> FASTA paths, the CPU oracle baseline and its comparison, "
                         "the strong sub-result of a multi-rank run (the --no-* switches above apply to these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's polished sequences and spans to DIR/*.npy (rank 0)")
    a = ap.parse_args()
    if a.repeats is None:
        a.repeats = 5 if a.full else 1
    if a.scaling == "strong":
        a.workload = "chr1"
    if a.workload == "chr1":
        a.scaling = "strong"
    if a.gpus > 1 and "RANK" not in os.environ:
        # not launched by torch.distributed.run: start the ranks ourselves (one process per GPU) and pass their line on
        return spawn_ranks(a.gpus)
    if a.scaling == "strong":
        return main_strong(a)

    import torch
    import torch.distributed as dist
    from nextpolish2_amd import Opts, Polisher
    from nextpolish2_amd.dist import SequenceGatherer
    from nextpolish2_amd.synth import Synth

    setup = dist_setup()
    rank, world, local_rank, dev, cdev, backend = setup
    if world != a.gpus and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    distributed = "RANK" in os.environ  # launched by torch.distributed.run (also with one rank: same code path)

    # synthetic inputs (SURVEY.md §8d recipe), one assembly per rank
    diploid = a.workload == "yeast"
    lengths = [max(20000, int(l * a.scale)) for l in (YEAST if diploid else [4_600_000])]
    ks = [21, 31] if diploid else [21]
    syn = make_assembly(lengths, a.depth, 1000 * rank + 1, diploid)
    yaks = [Synth.yak_assembly(syn, k) for k in ks]
    pol = Polisher(yaks, device=local_rank)
    contigs = [pol.upload(s.pileup) for s in syn]  # pileups resident in HBM before the timed region
    opts = Opts()
    groups = Groups(pol, contigs, lengths, max(1, min(a.groups, len(contigs))))
    total_len = sum(lengths)
    single = len(contigs) == 1  # one contig (configs[1]): the plain context path, output fetch deferred by one step
    gatherer = None
    if distributed:
        # RCCL all-gather of this rank's polished assembly, one per step, fed from the device: a contig's polished bytes
        # go from its slot context's result buffer into its slot of the staging buffer (device to device) as soon as its
        # batch group has delivered it; two staging buffers, because the groups may be one step ahead of the collective
        caps = [l + l // 16 + 1024 for l in lengths]
        gatherer = SequenceGatherer(sum(caps) + 16 * len(caps) + 4096, dev, collective_device=cdev, n_local=groups.ahead + 1)
        if not single:
            gatherer.set_slots(caps)

    pending = [False]
    last = [None]

    def step_single():
        _, span = pol.polish_resident(contigs[0], opts, want_pos=False, defer_output=True)
        if distributed:
            gatherer.gather_device(*pol.last_result_device())
        if pending[0]:
            last[0] = pol.fetch_end()  # the previous step's sequence is on the host now
        pol.fetch_begin()
        pending[0] = True
        return span

    def drain_single(span):
        if pending[0]:
            last[0] = pol.fetch_end()
            pending[0] = False
        return [(np.array(last[0]), span)]

    NB = groups.ahead + 1
    after = (lambda k, o: gatherer.gather_staged(k % NB, [len(x[0]) for x in o])) if distributed else None
    # a contig's polished bases reach the step's staging buffer by a copy the batch driver records itself (np2_batch_set_sink:
    # device to device, at the device-side length, inside the polish call); NP2_BENCH_STAGE_TORCH=1: by torch copies from the
    # slot contexts' result buffers after the call, as before (0.5 ms per step and rank more)
    stage = sink = None
    if distributed and os.environ.get("NP2_BENCH_STAGE_TORCH"):
        stage = lambda k, items: gatherer.stage(k % NB, items)
    elif distributed:
        sink = lambda k, i: gatherer.slot_address(k % NB, i)
    if os.environ.get("NP2_BENCH_NO_GATHER"):  # (experiment: the multi-rank launch without its per-step collective)
        after = stage = sink = None

    def sync():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    if single:
        for _ in range(a.warmup):
            out = step_single()
        if a.warmup:
            drain_single(out)
    elif a.warmup:
        groups.run(opts, a.warmup, after, stage=stage, sink=sink)
    groups.set_timing(True)  # HIP events around the batched k_diff_reads launches, on the batch streams
    diff_ms, diff_launches, call_ms = [], 0, 0.0
    import gc
    gc.collect()
    gc.disable()  # (the cyclic collector's pauses over the ctypes wrappers would be charged to the steps)
    # the set-up above (generators, uploads, warm-up) runs on dozens of host threads; in a container with a CPU quota the
    # timed region (20 steps = 90 ms) would otherwise start inside the same accounting period and be throttled for it
    time.sleep(float(os.environ.get("NP2_BENCH_SETTLE_S", "0.3")))
    sync()
    thr0 = cpu_throttle_stat()
    thr_cpu0 = thread_cpu_ns()
    cpu_t0 = time.process_time()
    t0 = time.perf_counter()
    if single:
        for _ in range(a.steps):
            out = step_single()
            tm = pol.timings()
            diff_ms.append(tm.get("diff_reads", 0.0))  # HIP events around k_diff_reads on the context's own stream
            if "diff_probe" in tm:  # (NP2_DENSE_PROBE: a part of the dense pass launched once more, tools/dense_probe.sh)
                print(f"diff_probe {tm['diff_probe']:.4f} ms (diff_reads {tm.get('diff_reads', 0.0):.4f})", file=sys.stderr)
            diff_launches = 1
    else:
        out, ms, diff_launches, call_ms = groups.run(opts, a.steps, after, stage=stage, sink=sink)
        call_breakdown = groups.call_breakdown
        diff_ms.append(ms)
    if single:
        out = drain_single(out)  # every polished sequence is on the host before the clock stops
    sync()
    dt = time.perf_counter() - t0
    cpu_dt = time.process_time() - cpu_t0
    thr1 = cpu_throttle_stat()
    thr_cpu1 = thread_cpu_ns()
    by_name = {}
    for tid, (ns, name) in thr_cpu1.items():
        d = ns - thr_cpu0.get(tid, (0, name))[0]
        if d > 0:
            e = by_name.setdefault(name, [0, 0.0])
            e[0] += 1
            e[1] += d / 1e9
    flush_log = [] if single else [b.flush_log() for b in groups.bps]
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, [o[0] for o in out], [o[1] for o in out])
    # the same region again (--repeats - 1 times, after the one the line's value comes from): boxes of the pool differ by
    # several per cent and a region is tens of milliseconds, so the line also carries the median and the spread
    region_dt = [dt]
    for _ in range(max(0, a.repeats - 1)):
        sync()
        t1 = time.perf_counter()
        if single:
            for _ in range(a.steps):
                o2 = step_single()
            drain_single(o2)
        else:
            groups.run(opts, a.steps, after, stage=stage, sink=sink)
        sync()
        region_dt.append(time.perf_counter() - t1)
    gc.enable()
    excl = None
    if a.full and not single and len(groups.bps) > 1 and not a.no_exclusive:  # the roofline kernel without other groups' kernels next to it (untimed)
        _, ms_x, k_x, _ = groups.run(opts, 2, None, exclusive=True)
        excl = (ms_x, k_x)
    groups.set_timing(False)
    bases = [np.array(o[0]) for o in out]
    spans = [o[1] for o in out]
    if distributed:
        t = torch.tensor(region_dt, dtype=torch.float64, device=cdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        region_dt = [float(x) for x in t.tolist()]
        dt = region_dt[0]

    total_bp = total_len
    if distributed:  # every rank polishes its own assembly: sum their lengths
        tb = torch.tensor([total_len], dtype=torch.int64, device=cdev)
        dist.all_reduce(tb, op=dist.ReduceOp.SUM)
        total_bp = int(tb.item())
    value = total_bp * a.steps / dt / 1e6
    total_bp_of = lambda rd, k: total_bp * k / float(np.median(rd)) / 1e6  # noqa: E731
    # roofline of the dominant kernel k_diff_reads (one batched launch per group and step): algorithmic bytes =
    # 0.5 B per streamed pileup column (packed nibbles, read once) + 0.5 B per contig base (nibble-packed contig)
    n_cols = sum(int(s.pileup.n_columns()) - s.pileup.L for s in syn)  # read 0 (the contig itself) is not streamed
    alg_bytes = 0.5 * n_cols + 0.5 * total_len  # per step = all launches of the step
    avg_ms = float(np.mean(diff_ms)) if diff_ms else 0.0
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
    n_reads = sum(s.pileup.n_reads for s in syn)

    wl = ("S. cerevisiae-sized diploid assembly: 17 contigs (S288C chromosome lengths, 12.16 Mb), 30x simulated HiFi "
          "(15x per haplotype), k21 + k31 yak, phasing on") if diploid else \
         "E. coli-sized contig, 30x simulated HiFi, k21 yak only"
    out_line = {
        "metric": "polished reference Mbp/s (whole node) at 30x HiFi + k21/k31; FASTA identical to oracle",
        "value": round(value, 3), "unit": "Mbp/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(dt / a.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "ms_per_step_regions": {"n": len(region_dt), "median": round(float(np.median(region_dt)) / a.steps * 1e3, 3),
                                "min": round(min(region_dt) / a.steps * 1e3, 3), "max": round(max(region_dt) / a.steps * 1e3, 3),
                                "value_at_median": round(total_bp_of(region_dt, a.steps), 3),
                                "note": "the same timed region repeated; `value` / `ms_per_step` are the FIRST region's"},
        "config": {"workload": wl + f", 1 assembly per MI355X", "contigs": len(lengths), "assembly_bp": total_len,
                   "depth": a.depth, "scale": a.scale, "reads": n_reads, "pileup_columns": int(n_cols), "yak_k": ks, "iter_count": 2,
                   "min_ctg_len": min(lengths), "batch_groups": 0 if single else len(groups.bps),
                   "parallelism": f"assembly-sharded x{world}; contigs batched per launch inside a GPU, batch groups on alternating-priority streams",
                   "output": "polished sequences copied to the host inside the step"},
        "roofline": {"bound": "hbm", "kernel": "k_diff_reads", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                     "traffic": PMC_TRAFFIC[a.workload] if (a.depth == 30 and a.scale == 1.0 and diff_launches == PMC_LAUNCHES[a.workload]) else None,
                     "traffic_source": f"not measured in this run: {PMC_SOURCE[a.workload]}, 2 x FETCH_SIZE + WRITE_SIZE per launch",
                     "alg_bytes_per_launch": int(alg_bytes / max(1, diff_launches)), "launches_per_step": diff_launches,
                     "avg_launch_ms": round(avg_ms / max(1, diff_launches), 4),
                     "units_per_launch_bp": int(total_len / max(1, diff_launches)),
                     "selected_by": "bytes (the kernel that streams the pileup), not time",
                     "time_share": (round(KERNEL_TIME[a.workload]["roofline_kernel_us"] / KERNEL_TIME[a.workload]["kernel_sum_us"], 4)
                                    if (a.depth == 30 and a.scale == 1.0) else None),
                     "time_dominant_kernel": ({"kernel": KERNEL_TIME[a.workload]["dominant_by_time"],
                                               "share": round(KERNEL_TIME[a.workload]["dominant_by_time_us"] / KERNEL_TIME[a.workload]["kernel_sum_us"], 4)}
                                              if (a.depth == 30 and a.scale == 1.0) else None),
                     "time_share_source": f"not measured in this run: {KERNEL_TIME[a.workload]['source']}"},
        "flush_ms": {"per_group_totals_host_issue_wait": [[round(sum(f[j] for f in fl), 3) for j in range(3)] for fl in flush_log],
                     "flushes_per_step": [len(fl) for fl in flush_log],
                     "per_flush_host_issue_wait_group0": flush_log[0] if flush_log else None,
                     "batch_call_ms_mean": round(float(call_ms), 3) if not single else None,
                     "call_breakdown_ms_per_group": None if single else call_breakdown},
        "host_cpu": {"cpu_seconds_per_wall_second": round(cpu_dt / dt, 2),
                     "by_thread_name": {k: {"threads": v[0], "cpus": round(v[1] / dt, 2)} for k, v in sorted(by_name.items(), key=lambda kv: -kv[1][1])[:8]},
                     "quota_periods_throttled_in_timed_region": None if not (thr0 and thr1) else thr1[1] - thr0[1],
                     "throttled_ms_in_timed_region": None if not (thr0 and thr1) else round((thr1[2] - thr0[2]) / 1e3, 2)},
    }

    if not single and len(groups.bps) > 1:
        out_line["roofline"]["note"] = ("one launch per batch group and step; in the timed region it shares the GPU with the other "
                                        "groups' kernels (roofline_exclusive: the same launches with the GPU to themselves; "
                                        "--workload ecoli: one contig, one stream)")
    if excl is not None and excl[0] > 0:
        # the same kernel over 2 extra, untimed steps in which the groups take turns: its launches then have the GPU to
        # themselves (in the timed region they share it with the other groups' kernels, which stretches them)
        ach_x = alg_bytes / (excl[0] * 1e-3) / 1e9
        out_line["roofline_exclusive"] = {"achieved": round(ach_x, 2), "frac": round(ach_x / HBM_PEAK_GBS, 5), "unit": "GB/s",
                                          "avg_launch_ms": round(excl[0] / max(1, excl[1]), 4), "launches_per_step": excl[1],
                                          "note": "one batch group at a time, outside the timed region"}
    if a.full and rank == 0 and world == 1 and not a.no_end_to_end:  # (N = 1 only; before the CPU baseline: its hundreds of threads leave the host noisy)
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            mid = sorted(range(len(syn)), key=lambda i: lengths[i])[len(syn) // 2]
            out_line["kernel_path_host_buffers"] = kernel_path_host_buffers(pol, syn, opts, bases)
            out_line["end_to_end"] = end_to_end(pol, syn[mid], yaks, opts, td, bases[mid])
            if not single and a.scale == 1.0:
                out_line["end_to_end_assembly"] = end_to_end_assembly(syn, yaks, td, bases, spans)
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:  # (the host-side baseline is reported at N = 1 only)
        # CPU baseline: the oracle (a port of the reference algorithm; the Rust reference cannot be built here)
        cb, oracle_out = cpu_baseline(syn, yaks, opts, a.cpu_threads)
        out_line["cpu_baseline"] = cb
        same = [bool(np.array_equal(ob, bases[i]) and (int(op[0]), int(op[-1])) == tuple(spans[i])) for i, (ob, op) in oracle_out.items()]
        out_line["fasta_identical_to_oracle"] = bool(len(same) == len(syn) and all(same))
        out_line["oracle_checked_contigs"] = len(same)
    # the path as a whole against the HBM roofline, by SURVEY.md §8(d)'s own formula: B bytes per polished bp =
    # iter_count x 0.5 B per pileup column (the reference streams the pileup once per pass) + 2 (contig in, consensus
    # out) + 8 B per k-mer table probe; achieved = Mbp/s x 1e6 x B
    kappa, ksrc = KAPPA[a.workload], KAPPA_SOURCE
    if "cpu_baseline" in out_line:
        kappa, ksrc = out_line["cpu_baseline"]["kmer_probes_per_bp"], "the oracle's kmer_probes stat, this run"
    b_per_bp = 2 * 0.5 * (n_cols + total_len) / total_len + 2 + 8 * kappa
    out_line["roofline_path"] = {"bound": "hbm", "what": "whole hot path (SURVEY.md 8d: achieved = Mbp/s x 1e6 x B)",
                                 "bytes_per_bp": round(b_per_bp, 3), "kappa_probes_per_bp": kappa, "kappa_source": ksrc,
                                 "achieved": round(value / max(1, world) * b_per_bp / 1e3, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                 "frac": round(value / max(1, world) * b_per_bp / 1e3 / HBM_PEAK_GBS, 5),
                                 "note": "per GPU; B = iter_count x 0.5 x pileup columns (read 0 included) / bp + 2 + 8 x kappa",
                                 "not_in_B": "SURVEY 8d's spill term (I x 40 x nu for graph nodes and scores kept in HBM) is 0 on the fused "
                                             "pass front: k_pf_tile keeps nodes, scores and the walk back in LDS; what passes between "
                                             "kernels per pass is 2 B/bp of per-tile consensus slots and 7 B/bp of consensus arrays "
                                             "(position, base, class, chain flag) - 18 B/bp per step, not counted in B"}
    if a.full and world > 1 and a.strong_mb > 0:
        # north_star's other curve — ONE assembly over the N GPUs: a diploid contig cut into N reference intervals, on the same
        # ranks, after the weak line's timed region (its own barrier + synchronize brackets; untouched by the value above)
        out_line["strong"] = strong_measure(a, setup, a.strong_mb, max(2, a.steps // 4), 1, True)
    import zlib
    out_line["output_crc32"] = zlib.crc32(b"".join(b.tobytes() for b in bases))  # rank 0's polished assembly (the same for every N)
    out_line["polished_equals_truth_contigs"] = int(sum(bases[i].tobytes() == syn[i].hap1 for i in range(len(syn))))
    if rank == 0:
        print(json.dumps(out_line), flush=True)
    if distributed:
        if rank == 0:
            # the gathered sequences really are the polished assemblies (checked outside the timed region)
            got = gatherer.to_host()
            assert got[0] == b"".join(b.tobytes() for b in bases), "all-gathered sequence differs from the polished assembly"
            assert all(len(got[r]) > 0 for r in range(world))
        dist.barrier()  # (rank 0 spends a while on the CPU baseline: leave together)
        dist.destroy_process_group()


if __name__ == "__main__":
    sys.exit(main() or 0)

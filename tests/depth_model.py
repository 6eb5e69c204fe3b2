"""The model the depth tests compare against: a BAM reader made of gzip and struct, the CIGAR measure and the admission
rule in numpy, np.add.at on a difference array, cumsum, and the runs read off the result.  tests/test_depth_cpu.py pins it
to known answers; tests/test_gpu_depth.py holds the device to it.  Nothing here touches the library."""
import gzip
import struct

import numpy as np

REC_DTYPE = np.dtype([("pos", "<i4"), ("flag", "<u2"), ("mapq", "u1"), ("pad", "u1"), ("n_cigar", "<u4"), ("pad2", "<u4"),
                      ("cigar_off", "<u8"), ("l_seq", "<u4"), ("pad3", "<u4"), ("seq_off", "<u8")])  # np2_bamrec_t
OPS = "MIDNSHP=X"
SPAN_OPS, ALIGNED_OPS, READ_OPS = "MDN=X", "MI=X", "MISH=X"
DEFAULTS = dict(min_depth=3, min_len=1000, min_aligned_fra=0.8, exclude_flags=0x4, min_mapq=0)


def cigar_words(ops):
    """[(op char, len)] -> BAM CIGAR words"""
    return [(int(n) << 4) | OPS.index(c) for c, n in ops]


def records(recs):
    """[(pos, flag, mapq, [(op, len)])] -> (REC_DTYPE array, uint32 CIGAR words)"""
    arr = np.zeros(len(recs), dtype=REC_DTYPE)
    cig = []
    for i, (pos, flag, mapq, ops) in enumerate(recs):
        arr[i]["pos"], arr[i]["flag"], arr[i]["mapq"] = pos, flag, mapq
        arr[i]["n_cigar"], arr[i]["cigar_off"] = len(ops), len(cig)
        cig.extend(cigar_words(ops))
    return arr, np.array(cig, dtype=np.uint32)


def read_bam(path):
    """-> (refs [(name, length)], {tid: (REC_DTYPE array, uint32 CIGAR words)}): BGZF blocks are gzip members"""
    with gzip.open(path, "rb") as f:
        data = f.read()
    assert data[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<I", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<I", data, o)
    o += 4
    refs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", data, o)
        refs.append((data[o + 4:o + 4 + l_name - 1].decode(), struct.unpack_from("<I", data, o + 4 + l_name)[0]))
        o += 8 + l_name
    per = {t: ([], []) for t in range(n_ref)}
    while o < len(data):
        bs, tid, pos, l_name, mapq, _bin, ncig, flag, l_seq = struct.unpack_from("<IiiBBHHHI", data, o)
        if tid >= 0:
            rows, cig = per[tid]
            rows.append((pos, flag, mapq, ncig, len(cig), l_seq))
            cig.extend(struct.unpack_from("<%dI" % ncig, data, o + 36 + l_name))
        o += 4 + bs
    out = {}
    for t, (rows, cig) in per.items():
        arr = np.zeros(len(rows), dtype=REC_DTYPE)
        for i, (pos, flag, mapq, ncig, coff, l_seq) in enumerate(rows):
            arr[i]["pos"], arr[i]["flag"], arr[i]["mapq"], arr[i]["n_cigar"], arr[i]["cigar_off"], arr[i]["l_seq"] = pos, flag, mapq, ncig, coff, l_seq
        out[t] = (arr, np.array(cig, dtype=np.uint32))
    return refs, out


def measure(recs, cigar):
    """per record (span, aligned, read_len) as int64 arrays"""
    n = len(recs)
    out = [np.zeros(n, np.int64) for _ in range(3)]
    nc = recs["n_cigar"].astype(np.int64)
    if n == 0 or nc.sum() == 0:
        return out
    rec_of = np.repeat(np.arange(n), nc)
    idx = np.concatenate([np.arange(int(o), int(o) + int(k)) for o, k in zip(recs["cigar_off"], nc) if k])
    w = cigar[idx].astype(np.int64)
    op, ln = w & 15, w >> 4
    for dst, ops in zip(out, (SPAN_OPS, ALIGNED_OPS, READ_OPS)):
        np.add.at(dst, rec_of, np.where(np.isin(op, [OPS.index(c) for c in ops]), ln, 0))
    return out


def counted_mask(recs, cigar, min_aligned_fra=0.8, exclude_flags=0x4, min_mapq=0, **_):
    span, aligned, read_len = measure(recs, cigar)
    ok = ((recs["flag"].astype(np.int64) & exclude_flags) == 0) & (recs["mapq"] >= min_mapq) & (recs["n_cigar"] > 0) & (read_len > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ok &= ~(aligned.astype(np.float64) / read_len.astype(np.float64) < min_aligned_fra)
    return ok, span


def all_runs(depth, min_depth):
    """every maximal run of depth >= min_depth as an (n, 2) int64 array of inclusive (s, e)"""
    ok = np.concatenate([[False], np.asarray(depth) >= min_depth, [False]])
    edge = np.flatnonzero(ok[1:] != ok[:-1])
    return np.stack([edge[0::2], edge[1::2] - 1], axis=1).astype(np.int64) if len(edge) else np.zeros((0, 2), np.int64)


def model(L, recs, cigar, **opts):
    """-> dict(depth, runs (kept, (n, 2) uint32), stats (the fields of np2_depth_stats_t but kernel_ms))"""
    o = dict(DEFAULTS, **opts)
    ok, span = counted_mask(recs, cigar, **o)
    pos = recs["pos"].astype(np.int64)
    ok_in = ok & (pos >= 0) & (pos < L)
    diff = np.zeros(L + 1, np.int64)
    np.add.at(diff, pos[ok_in], 1)
    np.add.at(diff, np.minimum(pos[ok_in] + np.maximum(span[ok_in], 1), L), -1)
    depth = np.cumsum(diff[:L])
    runs = all_runs(depth, o["min_depth"])
    kept = runs[(runs[:, 1] - runs[:, 0] + 1) >= o["min_len"]]
    stats = dict(records_seen=len(recs), records_counted=int(ok_in.sum()), sum_depth=int(depth.sum()), max_depth=int(depth.max()) if L else 0,
                 bases_ok=int((depth >= o["min_depth"]).sum()), runs=len(runs), runs_kept=len(kept),
                 bases_kept=int((kept[:, 1] - kept[:, 0] + 1).sum()))
    return dict(depth=depth.astype(np.uint32), runs=kept.astype(np.uint32), stats=stats)


# ---- what the module writes, formatted from a model ------------------------------------------------------------------------
def fasta_of(name, seq, runs):
    return b"".join(b">" + ("%s_%d_%d" % (name, s, e)).encode() + b"\n" + seq[s:e + 1].upper() + b"\n" for s, e in runs.tolist())


def bed_of(name, runs):
    return "".join("%s\t%d\t%d\n" % (name, s, e + 1) for s, e in runs.tolist())


def low_of(runs, L):
    """the complement of the kept runs inside [0, L), from a mask"""
    keep = np.zeros(L, bool)
    for s, e in runs.tolist():
        keep[s:e + 1] = True
    return all_runs((~keep).astype(np.int64), 1)


def bedgraph_of(name, depth):
    out, s = [], 0
    d = depth.tolist()
    for i in range(1, len(d) + 1):
        if i == len(d) or d[i] != d[s]:
            out.append("%s\t%d\t%d\t%d\n" % (name, s, i, d[s]))
            s = i
    return "".join(out)

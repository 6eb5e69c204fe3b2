"""The model the variant-caller tests compare against, written from the rule in include/np2_io.h (np2_varcall_*): a BAM reader
made of gzip and struct, a walk over every record's CIGAR in plain Python with numpy for the columns of an M run, a dict of
allele counts, and the call tests in Python integers.  It also formats the VCF and the summary the module writes.
tests/test_varcall_cpu.py pins it to hand-derived answers; tests/test_gpu_varcall.py holds the device to it.  Nothing here
touches the library."""
import gzip
import struct

import numpy as np

REC_DTYPE = np.dtype([("pos", "<i4"), ("flag", "<u2"), ("mapq", "u1"), ("pad", "u1"), ("n_cigar", "<u4"), ("pad2", "<u4"),
                      ("cigar_off", "<u8"), ("l_seq", "<u4"), ("pad3", "<u4"), ("seq_off", "<u8")])  # np2_bamrec_t
CALL_DTYPE = np.dtype([("pos", "<u4"), ("depth", "<u4"), ("count", "<u4"), ("pad0", "<u4"), ("bases", "<u8"), ("kind", "u1"),
                       ("gt", "u1"), ("len", "u1"), ("alt_code", "u1"), ("pad1", "<u4")])  # np2_varcall_t
OPS = "MIDNSHP=X"
M_OPS = (0, 7, 8)
DEFAULTS = dict(min_depth=8, min_alt=3, hom_pm=800, het_pm=250, max_indel=28, min_aligned_fra=0.0, exclude_flags=0xF04, min_mapq=5)
SNV, DEL, INS = 0, 1, 2
KINDS = ("SNV", "DEL", "INS")
CALL_KEYS = ("snv_het", "snv_hom", "del_het", "del_hom", "ins_het", "ins_hom")
STAT_KEYS = ("records_seen", "records_counted", "records_no_seq", "records_skipped", "events", "alleles", "callable") + CALL_KEYS
NIB = "=ACMGRSVTWYHKDBN"
REF_LUT = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    REF_LUT[ord(_c)] = REF_LUT[ord(_c.lower())] = _i
NIB_LUT = np.full(16, 4, np.uint8)
NIB_LUT[[1, 2, 4, 8]] = [0, 1, 2, 3]


def seq4_of(seq):
    """a read as text -> BAM 4-bit SEQ bytes (high nibble first)"""
    n = [NIB.index(c) if c in NIB else 15 for c in seq.upper()] + [0]
    return bytes((n[i] << 4) | n[i + 1] for i in range(0, len(seq), 2))


def records(recs):
    """[(pos, flag, mapq, [(op, len)], SEQ text or None for *)] -> (REC_DTYPE array, uint32 CIGAR words, uint8 SEQ bytes)"""
    arr = np.zeros(len(recs), dtype=REC_DTYPE)
    cig, seq = [], bytearray()
    for i, (pos, flag, mapq, ops, s) in enumerate(recs):
        arr[i]["pos"], arr[i]["flag"], arr[i]["mapq"] = pos, flag, mapq
        arr[i]["n_cigar"], arr[i]["cigar_off"] = len(ops), len(cig)
        cig.extend((int(n) << 4) | OPS.index(c) for c, n in ops)
        arr[i]["l_seq"], arr[i]["seq_off"] = len(s or ""), len(seq)
        seq += seq4_of(s or "")
    return arr, np.array(cig, dtype=np.uint32), np.frombuffer(bytes(seq), dtype=np.uint8)


def read_bam(path):
    """-> (refs [(name, length)], {tid: (REC_DTYPE array, uint32 CIGAR words, uint8 SEQ bytes)}): BGZF blocks are gzip members"""
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
    per = {t: ([], [], bytearray()) for t in range(n_ref)}
    while o < len(data):
        bs, tid, pos, l_name, mapq, _bin, ncig, flag, l_seq = struct.unpack_from("<IiiBBHHHI", data, o)
        if tid >= 0:
            rows, cig, seq = per[tid]
            rows.append((pos, flag, mapq, ncig, len(cig), l_seq, len(seq)))
            cig.extend(struct.unpack_from("<%dI" % ncig, data, o + 36 + l_name))
            s0 = o + 36 + l_name + 4 * ncig
            seq += data[s0:s0 + (l_seq + 1) // 2]
        o += 4 + bs
    out = {}
    for t, (rows, cig, seq) in per.items():
        arr = np.zeros(len(rows), dtype=REC_DTYPE)
        for i, row in enumerate(rows):
            arr[i]["pos"], arr[i]["flag"], arr[i]["mapq"], arr[i]["n_cigar"], arr[i]["cigar_off"], arr[i]["l_seq"], arr[i]["seq_off"] = row
        out[t] = (arr, np.array(cig, dtype=np.uint32), np.frombuffer(bytes(seq), dtype=np.uint8))
    return refs, out


def read_codes(seq4, seq_off, l_seq):
    b = np.asarray(seq4[seq_off:seq_off + (l_seq + 1) // 2], dtype=np.uint8)
    nib = np.empty(2 * len(b), np.uint8)
    nib[0::2], nib[1::2] = b >> 4, b & 15
    return NIB_LUT[nib[:l_seq]]


def reaches(c, d, pm):
    return c * 1000 >= pm * d


def judge(d, c, o):
    if d < o["min_depth"] or c < o["min_alt"] or not reaches(c, d, o["het_pm"]):
        return 0
    return 2 if reaches(c, d, o["hom_pm"]) else 1


def model(ref, recs, cigar, seq4, **opts):
    """-> dict(cov uint32 [L], alt uint32 [L, 4], calls (CALL_DTYPE), stats (STAT_KEYS), alleles {(anchor, kind, n, bases): count})"""
    o = dict(DEFAULTS, **opts)
    refc = REF_LUT[np.frombuffer(bytes(ref), dtype=np.uint8)]
    L = len(refc)
    diff = np.zeros(L + 1, np.int64)
    alt = np.zeros((L, 4), np.int64)
    st = dict.fromkeys(STAT_KEYS, 0)
    st["records_seen"] = len(recs)
    alleles = {}
    for r in recs:
        cg = [int(w) for w in cigar[int(r["cigar_off"]):int(r["cigar_off"]) + int(r["n_cigar"])]]
        ops = [(w & 15, w >> 4) for w in cg]
        span = sum(n for op, n in ops if op in (0, 2, 3, 7, 8))
        aligned = sum(n for op, n in ops if op in (0, 1, 7, 8))
        read_len = sum(n for op, n in ops if op in (0, 1, 4, 5, 7, 8))
        query = sum(n for op, n in ops if op in (0, 1, 4, 7, 8))
        pos = int(r["pos"])
        if (int(r["flag"]) & o["exclude_flags"]) or int(r["mapq"]) < o["min_mapq"] or not ops or read_len == 0:
            continue
        if np.float64(aligned) / np.float64(read_len) < o["min_aligned_fra"]:
            continue
        if pos < 0 or pos >= L:
            continue
        if any(op == 3 for op, _ in ops):
            st["records_skipped"] += 1
            continue
        if int(r["l_seq"]) != query:
            st["records_no_seq"] += 1
            continue
        st["records_counted"] += 1
        diff[pos] += 1
        diff[min(pos + max(span, 1), L)] -= 1
        rd = read_codes(seq4, int(r["seq_off"]), int(r["l_seq"]))
        p, q, m = pos, 0, 0  # m: columns of the M/=/X run that ends here
        for k, (op, n) in enumerate(ops):
            if op in M_OPS:
                cols = max(0, min(n, L - p))
                if cols:
                    rc, b = refc[p:p + cols], rd[q:q + cols]
                    hit = np.flatnonzero((rc < 4) & (b < 4) & (rc != b))
                    np.add.at(alt, (p + hit, b[hit]), 1)
                p, q, m = p + n, q + n, m + n
                continue
            if op in (1, 2) and 1 <= n <= o["max_indel"] and m >= 1 and 0 < k < len(ops) - 1 and ops[k - 1][0] in M_OPS and ops[k + 1][0] in M_OPS:
                a, qa, t = p - 1, q - 1, 0
                if op == 2 and a + n < L:
                    while t < m - 1 and refc[a - t] < 4 and refc[a - t] == refc[a - t + n] and rd[qa - t] == refc[a - t]:
                        t += 1
                    key = (a - t, 0, n, 0)
                    alleles[key] = alleles.get(key, 0) + 1
                    st["events"] += 1
                elif op == 1 and a + 1 < L and all(c < 4 for c in rd[qa + 1:qa + 1 + n]):
                    while t < m - 1 and rd[qa - t] < 4 and rd[qa - t] == rd[qa - t + n]:
                        t += 1
                    bases = 0
                    for c in rd[qa - t + 1:qa - t + 1 + n]:
                        bases = bases << 2 | int(c)
                    key = (a - t, 1, n, bases)
                    alleles[key] = alleles.get(key, 0) + 1
                    st["events"] += 1
            p += n if op in (2, 3) else 0
            q += n if op in (1, 4) else 0
            m = 0
    cov = np.cumsum(diff[:L])
    st["alleles"] = len(alleles)
    st["callable"] = int(((cov >= o["min_depth"]) & (refc < 4)).sum())
    best = {}  # (anchor, kind) -> (count, n, bases): the greatest count, then the smaller n, then the smaller bases
    for (a, kd, n, bases), c in alleles.items():
        cur = best.get((a, kd))
        if cur is None or (-c, n, bases) < (-cur[0], cur[1], cur[2]):
            best[(a, kd)] = (c, n, bases)
    calls = []
    for p in sorted(set(np.flatnonzero(alt.sum(axis=1)).tolist()) | {a for a, _ in best}):
        d = int(cov[p])
        if refc[p] < 4:
            b = int(np.argmax(alt[p]))  # (the first of the greatest: ties A < C < G < T; the reference base's count is 0)
            c = int(alt[p][b])
            gt = judge(d, c, o)
            if c and gt:
                calls.append((p, d, c, 0, 0, SNV, gt, 1, b, 0))
        for kd in (0, 1):
            if (p, kd) in best:
                c, n, bases = best[(p, kd)]
                d2 = min(d, int(cov[p + 1]) if p + 1 < L else 0)
                gt = judge(d2, c, o)
                if gt:
                    calls.append((p, d2, c, 0, bases, DEL if kd == 0 else INS, gt, n, 0, 0))
    for c in calls:
        st[CALL_KEYS[c[5] * 2 + c[6] - 1]] += 1
    return dict(cov=cov.astype(np.uint32), alt=alt.astype(np.uint32), calls=np.array(calls, dtype=CALL_DTYPE), stats=st, alleles=alleles)


# ---- what the module writes, formatted from a model ------------------------------------------------------------------------
VCF_META = ("##fileformat=VCFv4.2\n##source=nextpolish2_amd.varcall\n%s"
            "##INFO=<ID=KIND,Number=1,Type=String,Description=\"SNV, INS or DEL\">\n"
            "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Counted records covering the site\">\n"
            "##INFO=<ID=AC,Number=1,Type=Integer,Description=\"Counted records holding the called allele\">\n"
            "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"
            "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Counted records covering the site\">\n"
            "##FORMAT=<ID=AD,Number=1,Type=Integer,Description=\"Counted records holding the called allele\">\n"
            "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n")


def vcf_header_of(contigs):
    """contigs: [(name, length)]"""
    return VCF_META % "".join("##contig=<ID=%s,length=%d>\n" % c for c in contigs)


def vcf_of(name, ref, calls):
    out = []
    ref = bytes(ref).upper().decode()
    for c in calls.tolist():
        p, d, cnt, _, bases, kind, gt, n, b, _ = c
        if kind == SNV:
            r, a = ref[p], "ACGT"[b]
        elif kind == DEL:
            r, a = ref[p:p + 1 + n], ref[p]
        else:
            r, a = ref[p], ref[p] + "".join("ACGT"[(bases >> (2 * (n - 1 - i))) & 3] for i in range(n))
        out.append("%s\t%d\t.\t%s\t%s\t.\tPASS\tKIND=%s;DP=%d;AC=%d\tGT:DP:AD\t%s:%d:%d\n" % (name, p + 1, r, a, KINDS[kind], d, cnt, "1/1" if gt == 2 else "0/1", d, cnt))
    return "".join(out)


SUMMARY_HEADER = "#contig\tcallable\thom_snv\thom_ins\thom_del\thet_snv\thet_ins\thet_del\thom_per_mb\n"


def summary_of(rows):
    """rows: [(name, stats)] -> the per-contig rows and the total"""
    cols = ("callable", "snv_hom", "ins_hom", "del_hom", "snv_het", "ins_het", "del_het")
    tot = dict.fromkeys(cols, 0)
    out = [SUMMARY_HEADER]
    for name, st in rows + [("total", None)]:
        if st is None:
            st = tot
        else:
            for k in cols:
                tot[k] += st[k]
        hom = st["snv_hom"] + st["ins_hom"] + st["del_hom"]
        out.append("%s\t%s\t%.3f\n" % (name, "\t".join(str(int(st[k])) for k in cols), hom * 1e6 / st["callable"] if st["callable"] else 0.0))
    return "".join(out)

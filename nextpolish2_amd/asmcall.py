"""Call an assembly's differences from a reference on the GPU: the stretches of the reference that the assembly covers exactly
once (R) and the SNVs, deletions and insertions inside them (V), in the text layout of `paftools.js call`.  It is the third
over-correction measure of the reference's doc/benchmark5.md (step 6: minimap2 -cx asm10 --cs | sort | paftools.js call, then
e_use_vcf.py counts the calls that are not in a known set), and with a truth sequence as the reference it is "how many
differences from the truth", before and after a polish.

    python -m nextpolish2_amd.asmcall ref.fa[.gz] asm.fa[.gz] -o calls.txt[.gz] [--summary s.tsv] [--known known.vcf] [--host]

Every contig of the assembly is cut into segments of --seg (10000) bases that overlap by --overlap (2000, even); a contig
shorter than --seg is one segment, otherwise there are max(1, (Lc - overlap) // (seg - overlap)) segments and the last one runs
to the contig's end.  Segment i owns the part of it that is overlap / 2 away from its neighbours (the first from the contig's
start, the last to its end): the owned parts tile the contig.  The segments are mapped and aligned base by base to the
reference (the mapper and aligner of python -m nextpolish2_amd.map -a; --map_opts KEY=VAL,... as there, -k and -w), and every
alignment of mapping quality at least -q (5) that spans at least --min_aln (5000) reference bases contributes its owned part:
the reference positions it covers, and the differences the CIGAR shows there.  Positions covered exactly once make the R
lines; a difference is reported iff every position it touches is covered exactly once.  The rule is this project's own
(include/np2_io.h, np2_asmcall): equality with minimap2 and paftools is not claimed.

Text, tab-separated, coordinates 0-based half-open, alleles lower case in the reference's orientation; each reference's R lines,
then its V lines:
    R  ref  start  end
    V  ref  start  end  1  mapq  ref-allele|-  alt-allele|-  contig  qstart  qend  +|-
An SNV is [p, p + 1), a deletion after base a is [a + 1, a + 1 + n), an insertion after base a is [a + 1, a + 1).  A path ending
in .gz or .bgz is written as BGZF, compressed on the device.  --summary: per reference and in total, the R bases, the calls by
kind, the inserted and deleted bases, the segments (all, unmapped, mapped but not admitted) and the differences per Mb of R;
with --known, e_use_vcf.py's count: over the references the VCF names, a V line whose end is a POS of that reference in the
VCF is matched, any other is a potential error, and the rate is errors / R bases x 100.  --host runs the mapper's and the
caller's host twins (no kernel is launched for either).

Not here: asm10's scoring and the second affine gap piece; segments that map across structural rearrangements (they fail
--min_aln or -q and leave coverage 0); VCF output; several ranks; references or assemblies beyond one device's memory."""
import argparse
import os
import sys

SUMMARY_HEADER = "#ref\tr_bases\tsnv\tdel\tins\tins_bases\tdel_bases\tsegments\tunmapped\tnot_admitted\tdiff_per_mb"
KNOWN_HEADER = "\tmatched\tpotential_errors\terror_rate_pct"
BATCH_BYTES = 1 << 28  # contigs are handed to the mapper in batches of about this many segment bytes
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def tile(Lc, seg, overlap):
    """the segments of a contig of Lc bases -> [(start, end, own_lo, own_hi)] in contig coordinates"""
    m, step = overlap // 2, seg - overlap
    if Lc < seg:
        return [(0, Lc, 0, Lc)]
    n = max(1, (Lc - overlap) // step)
    out = []
    for i in range(n):
        s, e = i * step, (i * step + seg if i < n - 1 else Lc)
        out.append((s, e, 0 if i == 0 else s + m, Lc if i == n - 1 else s + seg - m))
    return out


def segment_alns(tiles, q_ids, recs, cigar_off, q_offs, cigar_base=0):
    """the aligner's records of the segments `tiles` (tile(...) rows, q_ids[i] their contig's number, q_offs[i] their first byte
    in the query stream) -> an api.ASMALN_DTYPE array; cigar_base: where this batch's CIGAR words start in the caller's array"""
    import numpy as np

    from .api import ASMALN_DTYPE
    a = np.zeros(len(tiles), ASMALN_DTYPE)
    t = np.asarray(tiles, dtype=np.int64).reshape(len(tiles), 4)
    for f in ("tid", "pos", "flag", "mapq", "n_cigar"):
        a[f] = recs[f]
    a["q_len"], a["own_lo"], a["own_hi"], a["q_base"] = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0], t[:, 3] - t[:, 0], t[:, 0]
    a["q_id"], a["q_off"] = q_ids, q_offs
    a["cigar_off"] = np.asarray(cigar_off[:len(tiles)], dtype=np.uint64) + np.uint64(cigar_base)
    return a


def run_text(name, runs):
    """R lines of one reference: `runs` the api.ASMRUN_DTYPE rows of it"""
    return "".join("R\t%s\t%d\t%d\n" % (name, s, e) for s, e in zip(runs["start"].tolist(), runs["end"].tolist()))


def var_text(name, ref, vars_, alns, query, contigs):
    """V lines of one reference: `ref` its bytes, `vars_` the api.ASMVAR_DTYPE rows of it, `alns` all alignments, `query` the
    query stream (bytes), `contigs` the contig names by q_id"""
    out = []
    for pos, ai, n, q_pos, kind, alt_code, rev in zip(*(vars_[f].tolist() for f in ("pos", "aln", "len", "q_pos", "kind", "alt_code", "rev"))):
        al = alns[ai]
        qs = int(al["q_base"]) + q_pos
        if kind == 0:
            s, e, r, alt, qe = pos, pos + 1, ref[pos:pos + 1].lower().decode(), "acgt"[alt_code], qs + 1
        elif kind == 1:
            s, e, r, alt, qe = pos + 1, pos + 1 + n, ref[pos + 1:pos + 1 + n].lower().decode(), "-", qs
        else:
            b = bytes(query[int(al["q_off"]) + q_pos:int(al["q_off"]) + q_pos + n])
            if rev:
                b = b.translate(_COMP)[::-1]
            s, e, r, alt, qe = pos + 1, pos + 1, "-", b.lower().decode("latin-1"), qs + n
        out.append("V\t%s\t%d\t%d\t1\t%d\t%s\t%s\t%s\t%d\t%d\t%s\n" % (name, s, e, int(al["mapq"]), r, alt, contigs[int(al["q_id"])], qs, qe, "-" if rev else "+"))
    return "".join(out)


def read_known(path):
    """a VCF -> {reference name: set of POS}"""
    import gzip
    known = {}
    with (gzip.open(path, "rt") if str(path).endswith(".gz") else open(path)) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            cells = line.split()
            known.setdefault(cells[0], set()).add(int(cells[1]))
    return known


def known_counts(known, name, r_bases, ends):
    """(matched, potential errors, R bases) of one reference under a known set; (0, 0, 0) when the set does not name it"""
    if name not in known:
        return 0, 0, 0
    matched = sum(1 for e in ends if e in known[name])
    return matched, len(ends) - matched, r_bases


def summary_text(rows, known=None):
    """rows: [(name, dict with r_bases, snv, del, ins, ins_bases, del_bases, segments, unmapped, not_admitted and, with `known`,
    matched, errors, known_bases)] -> one row per reference and the total (its unmapped segments belong to no reference)"""
    cols = ("r_bases", "snv", "del", "ins", "ins_bases", "del_bases", "segments", "unmapped", "not_admitted")
    kcols = ("matched", "errors", "known_bases")
    total = dict.fromkeys(cols + kcols, 0)
    for _, r in rows:
        for k in cols + (kcols if known is not None else ()):
            total[k] += int(r[k])
    out = [SUMMARY_HEADER + (KNOWN_HEADER if known is not None else "") + "\n"]
    for name, r in [x for x in rows if x[0] is not None] + [("total", total)]:
        n = int(r["snv"]) + int(r["del"]) + int(r["ins"])
        line = "%s\t%s\t%.3f" % (name, "\t".join(str(int(r[k])) for k in cols), n * 1e6 / int(r["r_bases"]) if int(r["r_bases"]) else 0.0)
        if known is not None:
            line += "\t%d\t%d\t%.6f" % (r["matched"], r["errors"], r["errors"] * 100.0 / r["known_bases"] if r["known_bases"] else 0.0)
        out.append(line + "\n")
    return "".join(out)


def build_parser():
    from .io import map_opts_arg
    p = argparse.ArgumentParser(prog="nextpolish2_amd.asmcall", description="call an assembly's differences from a reference: R and V lines as paftools.js call writes them")
    p.add_argument("ref", metavar="ref.fa[.gz]", help="the reference (or the truth sequence)")
    p.add_argument("asm", metavar="asm.fa[.gz]", help="the assembly")
    p.add_argument("-o", "--out", required=True, metavar="FILE", help="R and V lines; a name ending in .gz or .bgz is written as BGZF; an existing file is not overwritten")
    p.add_argument("--summary", default=None, metavar="FILE", help="per reference and in total: R bases, calls by kind, segments, differences per Mb")
    p.add_argument("--known", default=None, metavar="VCF", help="count the V lines whose end is not a POS of this VCF as potential errors (in --summary, or on standard error)")
    p.add_argument("--seg", type=int, default=10000, metavar="N", help="segment length [10000]")
    p.add_argument("--overlap", type=int, default=2000, metavar="N", help="overlap of neighbouring segments, even [2000]")
    p.add_argument("--min_aln", type=int, default=5000, metavar="N", help="admit an alignment only if it spans at least N reference bases [5000]")
    p.add_argument("-q", "--min_mapq", type=int, default=5, metavar="Q", help="admit an alignment only if its mapping quality is at least Q [5]")
    p.add_argument("-k", type=int, default=19, help="minimizer k-mer length [19]")
    p.add_argument("-w", type=int, default=19, help="minimizer window [19]")
    p.add_argument("--map_opts", type=map_opts_arg, default={}, metavar="KEY=VAL,...", help="the mapper's and aligner's options, as python -m nextpolish2_amd.map names them")
    p.add_argument("--host", action="store_true", help="run the mapper's and the caller's host twins")
    p.add_argument("--device", type=int, default=0)
    return p


def parse_args(argv=None):
    """every argument error stops here, before the library is loaded"""
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.overlap < 0 or a.overlap % 2:
        parser.error("--overlap: an even number >= 0")
    if not a.overlap < a.seg < 2 ** 31:
        parser.error("--seg: --overlap < N < 2^31")
    if not 0 <= a.min_aln < 2 ** 32:
        parser.error("--min_aln: 0 <= N < 2^32")
    if not 0 <= a.min_mapq <= 255:
        parser.error("--min_mapq: 0 <= Q <= 255")
    for k in ("k", "w"):
        if k in a.map_opts:
            parser.error(f"--map_opts: {k} is given with -{k}")
    for f in (a.ref, a.asm) + ((a.known,) if a.known else ()):
        if not os.path.isfile(f):
            parser.error(f"cannot open {f}")
    for f in (a.out, a.summary):
        if f is not None and os.path.exists(os.path.abspath(f)):
            raise SystemExit(f"Error: {os.path.abspath(f)!r} already exists!")
    return a


def align_segments(refs, contigs, seg=10000, overlap=2000, k=19, w=19, map_opts=None, host=False, device=0):
    """refs, contigs: [(name, bytes)] -> (alns as an api.ASMALN_DTYPE array, cigar words, the query stream): every contig's
    segments, mapped and aligned to the references, one MapIndex.align call (or map_align_host with host) per batch of contigs"""
    import numpy as np

    from . import api
    from . import io as np2io
    map_opts = dict(map_opts or {})
    ref_seqs = [s for _, s in refs]
    # batches of whole contigs; record i of a batch's result is its segment i
    batches, cur, cur_bytes = [], [], 0
    for ci, (_, s) in enumerate(contigs):
        cur.append(ci)
        cur_bytes += len(s)
        if cur_bytes >= BATCH_BYTES:
            batches.append(cur)
            cur, cur_bytes = [], 0
    if cur:
        batches.append(cur)
    index = None if host or not contigs else np2io.MapIndex(ref_seqs, k=k, w=w, device=device, stream=True, names=[n for n, _ in refs])
    alns, cigars, chunks, q_bytes, n_cig = [], [], [], 0, 0
    try:
        for batch in batches:
            tiles, q_ids, segs = [], [], []
            for ci in batch:
                for t in tile(len(contigs[ci][1]), seg, overlap):
                    tiles.append(t), q_ids.append(ci), segs.append(contigs[ci][1][t[0]:t[1]])
            if host:
                _, recs, cigar, cigar_off = np2io.map_align_host(ref_seqs, segs, k=k, w=w, **map_opts)
            else:
                _, recs, cigar, cigar_off = index.align(segs, **map_opts)
            lens = np.array([len(s) for s in segs], dtype=np.uint64)
            q_offs = q_bytes + np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
            alns.append(segment_alns(tiles, q_ids, recs, cigar_off, q_offs, n_cig))
            cigars.append(cigar), chunks.extend(segs)
            q_bytes += int(lens.sum())
            n_cig += len(cigar)
    finally:
        if index is not None:
            index.close()
    alns = np.concatenate(alns) if alns else np.zeros(0, api.ASMALN_DTYPE)
    cigar = np.concatenate(cigars) if cigars else np.zeros(0, np.uint32)
    return alns, cigar, b"".join(chunks)


def call(refs, contigs, seg=10000, overlap=2000, min_aln=5000, min_mapq=5, k=19, w=19, map_opts=None, host=False, device=0, pol=None,
         known=None):
    """refs, contigs: [(name, bytes)] -> (text, summary rows, stats): the module without its files.  `pol`: a Polisher to call on
    (one is made and closed otherwise; not used with host)."""
    import numpy as np

    from . import api
    alns, cigar, query = align_segments(refs, contigs, seg=seg, overlap=overlap, k=k, w=w, map_opts=map_opts, host=host, device=device)
    ref_seqs = [s for _, s in refs]
    if host:
        runs, vars_, st, _ = api.asmcall_host(ref_seqs, query, alns, cigar, min_mapq=min_mapq, min_aln=min_aln)
    else:
        own = pol is None
        pol = api.Polisher([], device=device) if own else pol  # (no k-mer table: the caller needs the device only)
        try:
            runs, vars_, st, _ = api.asmcall(pol, ref_seqs, query, alns, cigar, min_mapq=min_mapq, min_aln=min_aln)
        finally:
            if own:
                pol.close()
    # which segments are unmapped and which mapped but not admitted: the rule's admission over the aligner's records (it writes
    # M I D S only), its total checked against the library's
    unmapped = ((alns["flag"] & 4) != 0) | (alns["n_cigar"] == 0)
    ref_len = np.where(np.isin(cigar & 15, (0, 2, 7, 8)), cigar >> 4, 0).astype(np.int64)
    upto = np.concatenate(([0], np.cumsum(ref_len)))
    first = alns["cigar_off"].astype(np.int64)
    admitted = ~unmapped & (alns["mapq"] >= min_mapq) & (upto[first + alns["n_cigar"]] - upto[first] >= min_aln)
    if int(admitted.sum()) != st["alns_admitted"]:
        raise RuntimeError(f"the module admits {int(admitted.sum())} segments, the library {st['alns_admitted']}")
    text, rows = [], []
    contig_names = [n for n, _ in contigs]
    for t, (name, seq) in enumerate(refs):
        r, v = runs[runs["tid"] == t], vars_[vars_["tid"] == t]
        text.append(run_text(name, r))
        text.append(var_text(name, seq, v, alns, query, contig_names))
        mine, kind, n, pos = ~unmapped & (alns["tid"] == t), v["kind"], v["len"].astype(np.int64), v["pos"].astype(np.int64)
        row = {"r_bases": int((r["end"].astype(np.int64) - r["start"]).sum()), "snv": int((kind == 0).sum()), "del": int((kind == 1).sum()),
               "ins": int((kind == 2).sum()), "ins_bases": int(n[kind == 2].sum()), "del_bases": int(n[kind == 1].sum()), "segments": int(mine.sum()),
               "unmapped": 0, "not_admitted": int((mine & ~admitted).sum())}
        if known is not None:
            ends = pos + 1 + np.where(kind == 1, n, 0)  # a V line's end: p + 1, a + 1 + n, a + 1
            row["matched"], row["errors"], row["known_bases"] = known_counts(known, name, row["r_bases"], ends.tolist())
        rows.append((name, row))
    none = dict.fromkeys(("r_bases", "snv", "del", "ins", "ins_bases", "del_bases", "not_admitted", "matched", "errors", "known_bases"), 0)
    rows.append((None, dict(none, segments=int(unmapped.sum()), unmapped=int(unmapped.sum()))))  # (no reference's: counted in the total only)
    return "".join(text), rows, st


def main(argv=None):
    a = parse_args(argv)
    from . import io as np2io
    from .api import Np2Error
    known = read_known(os.path.abspath(a.known)) if a.known else None
    try:
        out = np2io.BgzfWriter(os.path.abspath(a.out), device=a.device) if np2io.is_bgzf_path(a.out) else open(os.path.abspath(a.out), "xb")
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    try:
        refs = list(np2io.read_fasta(os.path.abspath(a.ref)))
        contigs = list(np2io.read_fasta(os.path.abspath(a.asm)))
        text, rows, st = call(refs, contigs, seg=a.seg, overlap=a.overlap, min_aln=a.min_aln, min_mapq=a.min_mapq, k=a.k, w=a.w, map_opts=a.map_opts,
                              host=a.host, device=a.device, known=known)
        out.write(text.encode())
        summary = summary_text(rows, known)
        if a.summary is not None:
            with open(os.path.abspath(a.summary), "x") as f:
                f.write(summary)
        last = summary.rstrip("\n").split("\n")[-1].split("\t")
        sys.stderr.write("%d of %d segments admitted, %d R bases in %d runs, %d SNV, %d DEL, %d INS (%s per Mb)\n"
                         % (st["alns_admitted"], st["alns_seen"], st["r_bases"], st["runs"], st["kept_snv"], st["kept_del"], st["kept_ins"], last[10]))
        if known is not None:
            sys.stderr.write("Total matched variants: %s, Total potential errors: %s, potential error rate (%%): %s\n" % (last[11], last[12], last[13]))
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    finally:
        out.flush()
        out.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())

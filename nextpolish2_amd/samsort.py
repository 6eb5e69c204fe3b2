"""The mapper's SAM text, or BAM files in any order -> the coordinate-sorted BAM and its .bai: the `samtools sort -o
hifi.map.sort.bam -` and `samtools index` steps of the reference's recipe (and `samtools merge`, for several inputs), on the GPU.

Usage: python -m nextpolish2_amd.samsort map.sam[.gz]|in.bam|- [more ...] -o hifi.map.sort.bam [--sam_tie strand|input] [--full]

A BAM input (unsorted, sorted by name, one per SMRT cell: no index is read) is inflated and unpacked on the device; SAM and BAM
inputs may be mixed, and each file is sniffed on its own.  A BAM cannot come from standard input.
The text (plain or gzip; "-" is standard input) is parsed and sorted on the device (io.Sam with its names kept), the BAM
records are assembled there, compressed as BGZF there, and the index is derived there from the records' offsets and the
blocks' compressed sizes (include/np2_io.h has the rule: SAM specification 4.2 and 5.2; not compared with samtools' files).
Two kinds of file.  The lean BAM (the default) carries QNAME, FLAG, RNAME, POS, MAPQ, CIGAR and SEQ; QUAL is 0xFF, the mate
fields are unset, and the optional fields and the header lines other than @HD / @SQ are not carried.  It is what this
project's own readers need: -S (use_secondary), lowdepth and interval sharding.  The full BAM (--full) carries QUAL, RNEXT,
PNEXT, TLEN, every optional field (TAG:TYPE:VALUE to BAM's binary form, on the device) and the @RG / @PG / @CO lines too, for
tools that read base qualities or tags; the resident mapping then takes about three times the device memory.  Unmapped
records are dropped from both.  The [samsort] line says which kind was written."""
import argparse
import os
import sys
import time


def build_parser():
    from . import io as np2io
    p = argparse.ArgumentParser(prog="nextpolish2_amd.samsort", description="sort the mapper's SAM text into an indexed BAM on the GPU")
    p.add_argument("sam", nargs="+", metavar="map.sam[.gz]|in.bam|-",
                   help="SAM text, plain or gzip, or a BAM (sorted or not; no index is read); - is standard input (once, SAM text only)")
    p.add_argument("-o", "--out", required=True, metavar="hifi.map.sort.bam", help="the BAM; its index is written next to it as <out>.bai")
    p.add_argument("--sam_tie", choices=np2io.SAM_TIES, default="strand",
                   help="records at one position are ordered by strand, as samtools sort orders them, or stay in input order [strand]")
    p.add_argument("--full", action="store_true",
                   help="the full BAM: QUAL, RNEXT, PNEXT, TLEN, the optional fields and the @RG / @PG / @CO header lines are carried too "
                        "(about three times the device memory) [the lean BAM]")
    p.add_argument("--device", type=int, default=0)
    return p


def parse_args(argv=None):
    """every argument error stops here, before a device is touched"""
    parser = build_parser()
    a = parser.parse_args(argv)
    if a.sam.count("-") > 1:
        parser.error("standard input is given twice")
    for f in a.sam:
        if f != "-" and not os.path.isfile(f):
            parser.error(f"cannot open {f}")
    return a


def main(argv=None):
    a = parse_args(argv)
    from . import Polisher
    from . import io as np2io
    from .api import Np2Error
    t0 = time.time()
    pol = Polisher([], device=a.device)
    try:
        sam = np2io.Sam(pol, a.sam, tie=a.sam_tie, keep_names=True, keep_all=a.full)
        try:
            st = sam.write_bam(pol, a.out)
            parsed = sam.stats()
            ts = sam.tail_stats()
            bi = sam.bamin_stats()
        finally:
            sam.close()
    except Np2Error as e:
        raise SystemExit(f"Error: {e}")
    finally:
        pol.close()
    kind = f"full BAM ({ts['tail_bytes']} bytes of qualities, mate and optional fields)" if a.full else "lean BAM"
    print(f"[samsort] {kind}: {parsed['kept']} of {parsed['records']} records -> {a.out} ({st['file_bytes']} bytes, {st['blocks']} blocks) and "
          f"{a.out}.bai ({st['bins']} bins, {st['chunks']} chunks) in {time.time() - t0:.3f} s; kernels: emit {st['emit_ms']:.3f} ms, "
          f"deflate {st['deflate_ms']:.3f} ms, index {st['index_ms']:.3f} ms; {bi['files']} of {len(a.sam)} inputs were BAM"
          + (f" ({bi['records']} records of {bi['blocks']} blocks: inflate {bi['inflate_ms'] + bi['crc_ms']:.3f} ms, walk {bi['walk_ms']:.3f} ms, "
             f"pack {bi['fields_ms'] + bi['pack_ms']:.3f} ms)" if bi["files"] else ""), file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())

// The read front end: record admission (src/main.rs:1758-1817) and the GPU columnariser orchestration.
#include "np2_frontend.hpp"
#include "np2_iopool.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_sam.hpp"

namespace np2h {

// ---- record admission + GPU columnarisation (main.rs:1758-1817) -----------------------------------
void front_begin(np2_ctx *cx, const uint8_t *ref_glob, uint32_t L_in, const RecordSet &rs, const np2_front_opts_t *o, const ShardSpec *sp,
                 FrontWork &fw) {
    const np2_bamrec_t *recs = rs.recs;
    const uint32_t n_recs = rs.n_recs, *cigar = rs.cigar;
    const double t_a0 = np2h::now_ms();
    HIPCHK(hipSetDevice(cx->device));
    hipStream_t s = cx->stream;
    const uint32_t L_glob = L_in;                        // the contig (clip policy, contig-end checks)
    const uint32_t sub_lo = sp ? sp->sub_lo : 0u;
    const uint32_t L = sp ? sp->sub_hi - sp->sub_lo : L_in; // the (sub-)contig the pileup is built on
    const uint8_t *ref = ref_glob + sub_lo;
    if (L < 3) throw np2h::Np2Error(NP2_E_ARG, "contig too short");
    // the SEQ bytes are complete before anything else is: on their way to the device at once, next to the host work below
    // (69 MB of an E. coli-sized contig are 1.4 ms of bus time)
    np2h::DevBuf<uint8_t> d_seq;
    d_seq.cached = true;
    struct StreamIdleOnExit { // (d_seq goes back to the block cache when this function ends, however it ends)
        hipStream_t s;
        ~StreamIdleOnExit() { (void)hipStreamSynchronize(s); }
    } seq_guard{s};
    if (rs.seq_bytes && !rs.d_seq) {
        d_seq.ensure(rs.seq_bytes + 16);
        HIPCHK(hipMemcpyAsync(d_seq.p, rs.seq4, rs.seq_bytes, hipMemcpyHostToDevice, s));
    }
    // Admission + fill_with_cigar bookkeeping, in three steps over the host pool: (1) every record on its own — the
    // admission predicate (main.rs:1758-1771), the number of column-producing CIGAR ops, alignment columns, clipping;
    // (2) a prefix sum over the admitted records places their ops and their nibble slots; (3) the ops are written.  (One
    // thread walking 2 M CIGAR ops of an E. coli-sized contig was 3 of the 6.5 ms between the records and the pileup.)
    struct Pre {
        uint8_t admit = 0, is_clip = 0;
        int err = 0; // first offending condition of this record (NP2_E_*), message below
        const char *msg = nullptr;
        uint32_t n_ops = 0, col = 0;
    };
    std::vector<Pre> pre(n_recs);
    IoPool::get().parallel_for(((size_t)n_recs + 255) / 256, 64, [&](size_t blk) {
        for (uint32_t i = (uint32_t)blk * 256; i < std::min<uint64_t>(n_recs, ((uint64_t)blk + 1) * 256); ++i) {
            const np2_bamrec_t &r = recs[i];
            const uint32_t *cg = cigar + r.cigar_off;
            Pre &q = pre[i];
            uint64_t rlen = 0;
            int64_t span = 0;
            for (uint32_t k = 0; k < r.n_cigar; ++k) { // seq_len_from_cigar(true) / reference_end - reference_start
                const uint32_t l = cg[k] >> 4, op = cg[k] & 15;
                if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8 || op == 5) rlen += l;
                if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += l;
            }
            const bool secondary = r.flag & 0x100, supplementary = r.flag & 0x800;
            const int64_t need = std::max<int64_t>((int64_t)o->min_map_len, (int64_t)((float)rlen * o->min_map_fra));
            if ((r.flag & 0x404) != 0 || (int16_t)r.mapq <= o->min_map_qual || rlen <= o->min_read_len ||
                (secondary && !o->use_secondary) || (supplementary && !o->use_supplementary) || span < need)
                continue;
            // (-S: the record's SEQ must already be the one recovered from the read's primary alignment, main.rs:1775-1789;
            // np2_contig_from_bam does that, a caller of np2_contig_from_records passes it in)
            auto fail = [&](int code, const char *m) { q.err = code, q.msg = m; };
            if (r.pos < 0 || (uint32_t)r.pos > L_glob) { fail(NP2_E_REFPANIC, "reference would panic: record start outside the contig"); continue; }
            if (sp && (uint32_t)r.pos < sub_lo) { fail(NP2_E_ARG, "shard: record starts before the sub-contig"); continue; }
            // fill_with_cigar bookkeeping (main.rs:390-439): query clipping, columns
            uint32_t qs = 0, ts = 0, col = 0, aln_q_s = 0, aln_q_e = 0, n_ops = 0;
            bool is_first = true, bad_op = false;
            for (uint32_t k = 0; k < r.n_cigar; ++k) {
                const uint32_t l = cg[k] >> 4, op = cg[k] & 15;
                switch (op) {
                case 4:
                    qs += l;
                    if (is_first) aln_q_s = qs; else aln_q_e = qs - l;
                    break;
                case 0: case 7: case 8:
                    n_ops += l ? 1u : 0u;
                    col += l, qs += l, ts += l;
                    break;
                case 1:
                    n_ops += l ? 1u : 0u;
                    col += l, qs += l;
                    break;
                case 2:
                    n_ops += l ? 1u : 0u;
                    col += l, ts += l;
                    break;
                case 5:
                    break;
                default:
                    bad_op = true;
                }
                if (bad_op) break;
                is_first = false;
            }
            if (bad_op) { fail(NP2_E_REFPANIC, "reference would panic: Unknown cigar"); continue; }
            if (aln_q_e == 0) aln_q_e = qs;
            if (qs > r.l_seq) {
                fail(NP2_E_REFPANIC, secondary ? "reference would panic: no (or too short a) primary SEQ for a secondary alignment"
                                               : "reference would panic: SEQ shorter than CIGAR");
                continue;
            }
            if ((uint64_t)r.pos + ts > L_glob) { fail(NP2_E_REFPANIC, "reference would panic: alignment runs past the contig end"); continue; }
            if (sp && (uint64_t)r.pos + ts > sp->sub_hi) { fail(NP2_E_ARG, "shard: record ends behind the sub-contig"); continue; }
            if (r.seq_off + ((uint64_t)r.l_seq + 1) / 2 > rs.seq_bytes) { fail(NP2_E_ARG, "SEQ outside the buffer"); continue; }
            q.admit = 1;
            q.n_ops = n_ops, q.col = col;
            q.is_clip = aln_q_e - aln_q_s + o->max_clip_len < (uint32_t)rlen; // main.rs:1796-1797
        }
    });
    std::vector<FrontRec> frec;
    struct Admitted {
        uint32_t rec; // input record index
        bool is_clip;
    };
    std::vector<Admitted> adm;
    uint64_t out_off = ((((uint64_t)L + 1) >> 1) + 1 + 15) & ~15ull; // slot 0 = the contig itself
    uint64_t n_fops = 0;
    for (uint32_t i = 0; i < n_recs; ++i) { // (the first offending record in file order speaks, as in a sequential walk)
        const Pre &q = pre[i];
        if (q.err) throw np2h::Np2Error(q.err, q.msg);
        if (!q.admit) continue;
        // (pos, n_ops, op_off, seq_off, out_off, n_cols, pad)
        frec.push_back(FrontRec{(uint32_t)recs[i].pos - sub_lo, q.n_ops, n_fops, recs[i].seq_off, out_off, q.col, 0});
        adm.push_back(Admitted{i, q.is_clip != 0});
        n_fops += q.n_ops;
        out_off += ((((uint64_t)q.col + 1) >> 1) + 1 + 15) & ~15ull;
    }
    std::vector<FrontOp> fops(n_fops);
    IoPool::get().parallel_for((frec.size() + 63) / 64, 64, [&](size_t blk) {
        for (size_t a = blk * 64; a < std::min(frec.size(), (blk + 1) * 64); ++a) {
            const np2_bamrec_t &r = recs[adm[a].rec];
            const uint32_t *cg = cigar + r.cigar_off;
            FrontOp *dst = fops.data() + frec[a].op_off;
            uint32_t qs = 0, ts = 0, col = 0;
            for (uint32_t k = 0; k < r.n_cigar; ++k) {
                const uint32_t l = cg[k] >> 4, op = cg[k] & 15;
                switch (op) {
                case 4:
                    qs += l;
                    break;
                case 0: case 7: case 8:
                    if (l) *dst++ = FrontOp{col, qs, ts, (l << 4) | op};
                    col += l, qs += l, ts += l;
                    break;
                case 1:
                    if (l) *dst++ = FrontOp{col, qs, ts, (l << 4) | 1u};
                    col += l, qs += l;
                    break;
                case 2:
                    if (l) *dst++ = FrontOp{col, qs, ts, (l << 4) | 2u};
                    col += l, ts += l;
                    break;
                default:
                    break;
                }
            }
        }
    });
    const uint32_t n = (uint32_t)frec.size();
    const uint64_t nib_bytes = out_off + 64;
    const bool prof = getenv("NP2_IO_PROFILE") != nullptr;
    const double t_b0 = np2h::now_ms();
    double t_b1 = t_b0, t_b2 = t_b0;
    if (prof) fprintf(stderr, "  front_begin: admission + CIGAR prefix sums %.2f ms\n", t_b0 - t_a0);

    np2_contig *c = fw.c = new np2_contig();
    {
        c->nib.ensure(nib_bytes + 64); // every slot is written completely by its producer kernel
        np2h::DevBuf<uint8_t> d_ref;
        np2h::DevBuf<FrontRec> d_rec;
        np2h::DevBuf<FrontOp> d_ops;
        np2h::DevBuf<FrontOut> d_out;
        d_ref.cached = d_rec.cached = d_ops.cached = d_out.cached = true; // (released after the read-back below)
        d_ref.ensure(L + 16);
        HIPCHK(hipMemcpyAsync(d_ref.p, ref, L, hipMemcpyHostToDevice, s));
        launch_pack_ref(s, d_ref.p, L, c->nib.p);
        std::vector<FrontOut> fout(n);
        if (n) {
            if (!rs.d_seq) d_seq.ensure(rs.seq_bytes + 16); // (already there unless the records carry no SEQ at all)
            d_rec.ensure(n);
            d_ops.ensure(fops.size() + 1);
            d_out.ensure(n);
            t_b1 = np2h::now_ms();
            HIPCHK(hipMemcpyAsync(d_rec.p, frec.data(), (size_t)n * sizeof(FrontRec), hipMemcpyHostToDevice, s));
            HIPCHK(hipMemcpyAsync(d_ops.p, fops.data(), fops.size() * sizeof(FrontOp), hipMemcpyHostToDevice, s));
            {
                np2h::EventTimer t(cx, "columnarise");
                launch_columnarise(s, d_rec.p, n, d_ops.p, d_ref.p, rs.d_seq ? rs.d_seq : d_seq.p, c->nib.p, d_out.p);
            }
            fout = np2h::d2h(cx, d_out.p, n);
            t_b2 = np2h::now_ms();
        } else {
            HIPCHK(hipStreamSynchronize(s));
        }
        // keep / drop / label (main.rs:1798-1813), then filter_alignseqs_by_clip (531-574)
        std::vector<np2_read_t> &reads = fw.reads;
        std::vector<uint8_t> &lable = fw.lable;
        np2_read_t r0;
        memset(&r0, 0, sizeof r0);
        r0.aln_t_s = 0, r0.aln_t_e = L - 1, r0.nib_off = 0, r0.n_cols = L;
        reads.push_back(r0);
        lable.push_back(0);
        std::vector<uint8_t> pushed(n_recs, 0);
        std::vector<uint32_t> &rec_of = fw.rec_of;
        rec_of.assign(1, 0);
        for (uint32_t i = 0; i < n; ++i) {
            if (fout[i].n_cols <= o->min_map_len) continue; // aln_len() <= min_map_len
            if (adm[i].is_clip && L_glob < 500000) continue;
            pushed[adm[i].rec] = 1;
            rec_of.push_back(adm[i].rec);
            np2_read_t rd;
            memset(&rd, 0, sizeof rd);
            rd.aln_t_s = fout[i].aln_t_s;
            rd.aln_t_e = fout[i].aln_t_e;
            rd.n_cols = fout[i].n_cols;
            rd.nib_off = frec[i].out_off;
            reads.push_back(rd);
            lable.push_back(adm[i].is_clip ? 1 : 0);
        }
        {
            // the sortedness assertion compares every record with the start of the last record that was *pushed*
            // (pre_pos only advances at main.rs:1814-1815, after the trim-length and short-contig clip skips)
            int64_t pre_pos = 0;
            for (uint32_t i = 0; i < n_recs; ++i) {
                if (recs[i].pos < pre_pos) throw np2h::Np2Error(NP2_E_REFPANIC, "reference would panic: Unsorted input file!");
                if (pushed[i]) pre_pos = recs[i].pos;
            }
        }
        if (sp) {
            // reads that do not reach the shard's zone keep their number but are not held (like np2_shard_upload)
            for (size_t i = 1; i < reads.size(); ++i) {
                const uint32_t gs = reads[i].aln_t_s + sub_lo, ge = reads[i].aln_t_e + sub_lo;
                if (ge < sp->zone_lo || gs >= sp->zone_hi) {
                    reads[i].flags |= NP2_READ_DROPPED;
                    reads[i].n_cols = 0;
                    lable[i] = 0;
                }
            }
        }
        fw.nib_bytes = nib_bytes;
        fw.L = L, fw.L_glob = L_glob, fw.sub_lo = sub_lo;
    }
    if (prof)
        fprintf(stderr, "  front_begin: device allocations %.2f ms, H2D + columnarise + read-back %.2f ms, keep/drop + temp frees %.2f ms\n",
                t_b1 - t_b0, t_b2 - t_b1, np2h::now_ms() - t_b2);
}

void front_finish(np2_ctx *cx, FrontWork &fw, np2_contig **out) {
    const double t_c0 = np2h::now_ms();
    np2_contig *c = fw.c;
    std::vector<np2_read_t> &reads = fw.reads;
    std::vector<uint8_t> &lable = fw.lable;
    const uint32_t L = fw.L, L_glob = fw.L_glob, sub_lo = fw.sub_lo;
    const uint64_t nib_bytes = fw.nib_bytes;
    // (a shard applies the clip filter in contig coordinates: entry 0 is the whole contig there)
    const uint32_t offset = 50;
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    std::vector<size_t> clip_dropped;
    uint32_t rs = 0, re = 0;
    for (size_t i = 0; i < reads.size(); ++i) {
        if (lable[i] || (reads[i].flags & NP2_READ_DROPPED)) continue;
        const uint32_t ts = (i == 0 ? 0u : reads[i].aln_t_s + sub_lo) + offset;
        const uint32_t te = (i == 0 ? L_glob - 1 : reads[i].aln_t_e + sub_lo) - offset;
        if (rs == re) {
            rs = ts, re = te;
        } else if (ts > re) {
            ranges.emplace_back(rs, re);
            rs = ts, re = te;
        } else if (re < te) {
            re = te;
        }
    }
    if (rs != re) ranges.emplace_back(rs, re);
    for (size_t i = 0; i < reads.size(); ++i) {
        if (!lable[i]) continue;
        const uint32_t gs = reads[i].aln_t_s + sub_lo, ge = reads[i].aln_t_e + sub_lo;
        for (auto &rg : ranges) {
            if (rg.first <= gs && ge <= rg.second) {
                reads[i].flags |= NP2_READ_DROPPED; // align_bases = Vec::new(), index retained
                reads[i].n_cols = 0;
                clip_dropped.push_back(i);
                break;
            } else if (ge < rg.first) {
                break;
            }
        }
    }
    // a slot emptied by the clip filter still needs a terminator in its (unused) stream
    for (size_t i : clip_dropped) {
        const uint8_t ff = 0xFF;
        np2h::h2d_staged(cx, c->nib.p + reads[i].nib_off, &ff, 1);
    }
    const double t_c1 = np2h::now_ms();
    np2h::finish_contig(cx, c, reads.data(), (uint32_t)reads.size(), L, nib_bytes);
    if (getenv("NP2_IO_PROFILE"))
        fprintf(stderr, "  front_finish: clip filter %.2f ms, finish_contig (descriptors, tile read lists, uploads) %.2f ms\n",
                t_c1 - t_c0, np2h::now_ms() - t_c1);
    fw.c = nullptr; // handed over
    *out = c;
}

static void contig_from_records(np2_ctx *cx, const uint8_t *ref, uint32_t L, const RecordSet &rs, const np2_front_opts_t *o, np2_contig **out) {
    FrontWork fw;
    front_begin(cx, ref, L, rs, o, nullptr, fw);
    front_finish(cx, fw, out);
}

// the front end for the SAM reader (np2_sam_host.cpp): its SEQ bytes are resident, its records and CIGAR words come from the host
void contig_from_device_seq(np2_ctx *cx, const uint8_t *ref, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs, const uint32_t *cigar,
                            const uint8_t *d_seq4, uint64_t seq4_bytes, const np2_front_opts_t *opts, np2_contig **out) {
    RecordSet rs;
    rs.recs = recs, rs.cigar = cigar, rs.n_recs = n_recs;
    rs.device_seq(d_seq4, seq4_bytes);
    contig_from_records(cx, ref, L, rs, opts, out);
}

} // namespace np2h

extern "C" {

int np2_contig_from_records(np2_ctx_t *cx, const uint8_t *ref, uint32_t L, const np2_bamrec_t *recs, uint32_t n_recs,
                            const uint32_t *cigar, const uint8_t *seq4, const np2_front_opts_t *opts,
                            np2_contig_t **out) {
    if (!cx || !ref || !opts || !out) return NP2_E_ARG;
    *out = nullptr;
    return np2h::abi_guard([&] {
        np2h::RecordSet rs;
        rs.recs = recs, rs.cigar = cigar, rs.n_recs = n_recs, rs.seq4 = seq4;
        for (uint32_t i = 0; i < n_recs; ++i) rs.seq_bytes = std::max<uint64_t>(rs.seq_bytes, recs[i].seq_off + ((uint64_t)recs[i].l_seq + 1) / 2);
        np2h::contig_from_records(cx, ref, L, rs, opts, out);
        np2h::flush_timings(cx);
        return NP2_OK;
    }, np2h::ctx_sink(cx, true));
}

int np2_contig_export(np2_ctx_t *cx, np2_contig_t *c, np2_read_t **reads, uint32_t *n_reads, uint8_t **nibbles,
                      uint64_t *nib_bytes) {
    if (!cx || !c || !reads || !n_reads || !nibbles || !nib_bytes) return NP2_E_ARG;
    return np2h::abi_guard([&] {
        HIPCHK(hipSetDevice(cx->device));
        *reads = (np2_read_t *)malloc((size_t)c->R * sizeof(np2_read_t));
        *nibbles = (uint8_t *)malloc(c->nib_bytes);
        HIPCHK(hipMemcpy(*reads, c->reads.p, (size_t)c->R * sizeof(np2_read_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(*nibbles, c->nib.p, c->nib_bytes, hipMemcpyDeviceToHost));
        *n_reads = c->R;
        *nib_bytes = c->nib_bytes;
        return NP2_OK;
    }, np2h::ctx_sink(cx));
}
}

// What every producer of a resident SAM handle shares: the input-order arrays that grow while records come in, and the one
// path from them to the handle's sorted arrays.  np2_sam_host.cpp fills them from SAM text and BAM pieces (its Build adds the
// parsing), np2_map_host.cpp from the aligner's records (np2_sam_from_reads).  All device work runs on the stream given.
#pragma once
#include "np2_ctx.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_kernels.hpp"
#include "np2_sam.hpp"
#include "np2_sam_handle.hpp"

namespace np2h {

// room for `bytes` more on the device, or NP2_E_NOMEM saying how much was needed
inline void need_device(size_t bytes, const char *what) {
    need_device_bytes(bytes, (size_t)64 << 20, [&](size_t fr) {
        return std::string("the SAM's ") + what + " need a block of " + std::to_string(bytes) + " bytes, and the device has " +
               std::to_string(fr) + " bytes free: the packed SEQ, the CIGAR words and the records of a SAM input must fit one device's memory";
    });
}
template <class T> void take_over(DevBuf<T> &a, DevBuf<T> &b) { // a <- b's block, b <- a's
    std::swap(a.p, b.p), std::swap(a.cap, b.cap), std::swap(a.cached, b.cached), std::swap(a.cache_bytes, b.cache_bytes),
        std::swap(a.slab_bytes, b.slab_bytes);
}
// `b` holds `used` elements and gets room for `need`: a larger block and a device-to-device copy, as SeqStream::push grows
template <class T> void grow(DevBuf<T> &b, size_t used, size_t need, hipStream_t st, const char *what) {
    if (need <= b.cap) return;
    const size_t want = std::max(need, b.cap + b.cap / 2);
    need_device((want + want / 8 + 64) * sizeof(T), what);
    DevBuf<T> nb;
    nb.cached = true;
    nb.ensure(want);
    if (used) HIPCHK(hipMemcpyAsync(nb.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipStreamSynchronize(st)); // (the old block goes back to the cache: nothing may still read it)
    take_over(b, nb);
}

struct SamAccum {
    np2_sam &sam;
    hipStream_t st;
    // input order, while the records come in
    DevBuf<uint32_t> recs_in, cigar_in;
    DevBuf<int32_t> tids_in;
    DevBuf<uint64_t> keys_in;
    uint64_t n_recs = 0, n_cigar = 0, seq_bytes = 0, n_records = 0;
    // NP2_SAM_KEEP_NAMES: offset << 8 | length of each record's name, input order
    bool keep_names = false;
    DevBuf<uint64_t> nref_in;
    uint64_t name_bytes = 0;
    // NP2_SAM_KEEP_ALL: offset << 1 | has_qual of each record's tail, input order
    bool keep_all = false;
    DevBuf<uint64_t> tref_in;
    uint64_t tail_bytes = 0;
    DevBuf<uint8_t> d_tmp;
    DevEvent e0, e1;

    SamAccum(np2_sam &s, hipStream_t stream) : sam(s), st(stream) {
        recs_in.cached = cigar_in.cached = tids_in.cached = keys_in.cached = true; // (every release below follows a drained stream)
        nref_in.cached = tref_in.cached = d_tmp.cached = true;
        e0.make(), e1.make();
    }
    ~SamAccum() { (void)hipStreamSynchronize(st); } // (work on the input-order arrays may be in flight when an error unwinds the owner)

    // `kept` more records with n_cig CIGAR words fit the handle's limits
    void check_room(uint64_t kept, uint64_t n_cig) const {
        if (n_recs + kept >= (1ull << 31)) throw Np2Error(NP2_E_UNSUPPORTED, "a SAM input of 2^31 alignment records or more");
        if (n_cigar + n_cig >= 0xFFFF0000ull) throw Np2Error(NP2_E_UNSUPPORTED, "a SAM input of more than 4294901760 CIGAR operations");
    }
    // room behind what is held for `kept` more records: n_cig words, n_seq SEQ bytes, n_name name bytes, n_tail tail bytes
    void reserve(uint64_t kept, uint64_t n_cig, uint64_t n_seq, uint64_t n_name, uint64_t n_tail) {
        if (keep_names) {
            grow(nref_in, n_recs, n_recs + kept, st, "names");
            grow(sam.names, name_bytes, name_bytes + n_name + 1, st, "names");
        }
        if (keep_all) {
            grow(tref_in, n_recs, n_recs + kept, st, "tails");
            grow(sam.tails, tail_bytes, tail_bytes + n_tail + 16, st, "quality bytes and optional fields");
        }
        grow(recs_in, n_recs * np2::SAM_REC_WORDS, (n_recs + kept) * np2::SAM_REC_WORDS, st, "records");
        grow(tids_in, n_recs, n_recs + kept, st, "records");
        grow(keys_in, n_recs, n_recs + kept, st, "sort keys");
        grow(cigar_in, n_cigar, n_cigar + n_cig + 1, st, "CIGAR words");
        grow(sam.seq4, seq_bytes, seq_bytes + n_seq + 16, st, "packed SEQ");
    }
    void advance(uint64_t kept, uint64_t n_cig, uint64_t n_seq, uint64_t n_name, uint64_t n_tail) {
        n_recs += kept, n_cigar += n_cig, seq_bytes += n_seq, name_bytes += n_name, tail_bytes += n_tail;
    }

    // after the last record: input order -> sorted order
    void finish() {
        const uint32_t n = (uint32_t)n_recs;
        sam.n_recs = n_recs, sam.n_cigar = n_cigar, sam.seq_bytes = seq_bytes;
        sam.has_names = keep_names, sam.name_bytes = name_bytes;
        sam.has_tails = keep_all, sam.tail_bytes = tail_bytes;
        if (tail_bytes) HIPCHK(hipMemsetAsync(sam.tails.p + tail_bytes, 0, 16, st)); // (the encoder reads whole words)
        sam.stats.records = n_records, sam.stats.kept = n_recs, sam.stats.unmapped = n_records - n_recs;
        sam.stats.cigar_words = n_cigar, sam.stats.seq_bytes = seq_bytes;
        if (seq_bytes) HIPCHK(hipMemsetAsync(sam.seq4.p + seq_bytes, 0, 16, st)); // (what records_to_arrays appends, for a reader of 16-byte words)
        if (n == 0) {
            HIPCHK(hipStreamSynchronize(st));
            return;
        }
        const size_t tmp_bytes = np2::prim_temp_bytes((size_t)n + 1);
        need_device((size_t)n * (8 + 4 + 4 + 4 + 4 + 4 + 40 + (keep_names ? 8 : 0) + (keep_all ? 8 : 0)) + (n_cigar + 1) * 4 + tmp_bytes, "sorted records and CIGAR words");
        DevBuf<uint64_t> keys_out;
        DevBuf<uint32_t> vals_in, vals_out, sizes, offs;
        keys_out.cached = vals_in.cached = vals_out.cached = sizes.cached = offs.cached = true; // (released after the last synchronisation below)
        keys_out.ensure(n), vals_in.ensure(n), vals_out.ensure(n), sizes.ensure((size_t)n + 1), offs.ensure((size_t)n + 1);
        d_tmp.ensure(tmp_bytes);
        sam.recs.ensure((size_t)n * np2::SAM_REC_WORDS), sam.tids.ensure(n), sam.cigar.ensure(n_cigar + 1);
        HIPCHK(hipEventRecord(e0.e, st));
        np2::launch_sam_iota(st, vals_in.p, n);
        if (np2::prim_sort_pairs_u64_u32(st, d_tmp.p, tmp_bytes, keys_in.p, keys_out.p, vals_in.p, vals_out.p, n, 64))
            throw Np2Error(NP2_E_DEVICE, "rocprim radix_sort_pairs failed");
        np2::launch_sam_sorted_sizes(st, recs_in.p, vals_out.p, n, sizes.p);
        if (np2::prim_exclusive_sum_u32(st, d_tmp.p, tmp_bytes, sizes.p, offs.p, (size_t)n + 1))
            throw Np2Error(NP2_E_DEVICE, "rocprim exclusive_scan failed");
        np2::launch_sam_gather(st, recs_in.p, tids_in.p, cigar_in.p, vals_out.p, offs.p, n, sam.recs.p, sam.tids.p, sam.cigar.p);
        if (keep_names) {
            sam.name_ref.ensure(n);
            np2::launch_sam_gather_u64(st, nref_in.p, vals_out.p, n, sam.name_ref.p);
        }
        if (keep_all) {
            sam.tail_ref.ensure(n);
            np2::launch_sam_gather_u64(st, tref_in.p, vals_out.p, n, sam.tail_ref.p);
        }
        HIPCHK(hipEventRecord(e1.e, st));
        sam.keys.resize(n);
        HIPCHK(hipMemcpyAsync(sam.keys.data(), keys_out.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        sam.stats.sort_ms = elapsed(e0, e1);
    }
};

} // namespace np2h

// The host twin of the aligner-to-handle packing (include/np2_io.h: np2_align_pack_host): uses no device and no HIP header, so
// that a plain C++ compiler builds it (tests/tools/alnpack_core_test.cpp).  The rule's text is np2_alnpack_core.hpp.
#if defined(__HIPCC__) // (the library's build compiles every source as HIP: the core headers' qualifiers need its runtime header)
#include <hip/hip_runtime.h>
#endif

#include "../../include/np2_io.h"
#include "np2_abi.hpp"
#include "np2_alnpack_core.hpp"

#include <cstdlib>

namespace np2h {
int io_set_error(int code, const std::string &msg); // the entry points' message slot (np2_io.cpp); returns `code`
}

static_assert(sizeof(np2_align_rec_t) == sizeof(np2aln::Rec), "np2_align_rec_t is np2aln::Rec");
static_assert(sizeof(np2_bamrec_t) == np2pack::REC_WORDS * 4, "np2_bamrec_t is written word by word");

namespace {
template <class T> T *to_malloc(const std::vector<T> &v) { // NULL when empty
    if (v.empty()) return nullptr;
    T *p = (T *)malloc(v.size() * sizeof(T));
    if (!p) throw np2h::Np2Error(NP2_E_NOMEM, "np2_align_pack_host: out of memory");
    memcpy((void *)p, v.data(), v.size() * sizeof(T));
    return p;
}
} // namespace

extern "C" int np2_align_pack_host(const np2_align_rec_t *recs, const uint32_t *cigar, const uint64_t *cigar_off, const uint8_t *reads, uint64_t n,
                                   uint64_t n_reads, const np2_sam_opts_t *sam_opts, np2_bamrec_t **out_recs, int32_t **tids, uint32_t **out_cigar,
                                   uint8_t **seq4, uint64_t *n_recs) {
    return np2h::abi_guard([&] {
        using np2h::Np2Error;
        if (!out_recs || !tids || !out_cigar || !seq4 || !n_recs) throw Np2Error(NP2_E_ARG, "np2_align_pack_host: NULL argument");
        *out_recs = nullptr, *tids = nullptr, *out_cigar = nullptr, *seq4 = nullptr, *n_recs = 0;
        if ((n_reads && (!recs || !cigar_off)) || (n && !reads)) throw Np2Error(NP2_E_ARG, "np2_align_pack_host: NULL argument");
        for (uint64_t i = 0; i < n_reads; ++i)
            if (cigar_off[i + 1] - cigar_off[i] != recs[i].n_cigar || (recs[i].n_cigar && !cigar))
                throw Np2Error(NP2_E_ARG, "np2_align_pack_host: cigar_off does not follow the records' n_cigar (read " + std::to_string(i) + ")");
        std::vector<uint32_t> r, c;
        std::vector<int32_t> t;
        std::vector<uint8_t> s;
        if (!np2pack::pack_host(reinterpret_cast<const np2aln::Rec *>(recs), cigar, cigar_off, reads, n, n_reads,
                                sam_opts ? (sam_opts->tie_by_strand ? 1u : 0u) : 1u, r, t, c, s))
            throw Np2Error(NP2_E_ARG, "np2_align_pack_host: the read stream does not hold n_reads newline-terminated reads");
        uint32_t *pr = nullptr, *pc = nullptr;
        int32_t *pt = nullptr;
        try {
            pr = to_malloc(r), pt = to_malloc(t), pc = to_malloc(c);
            *seq4 = to_malloc(s);
        } catch (...) {
            free(pr), free(pt), free(pc);
            throw;
        }
        *out_recs = reinterpret_cast<np2_bamrec_t *>(pr), *tids = pt, *out_cigar = pc, *n_recs = t.size();
        return NP2_OK;
    }, np2h::io_set_error);
}

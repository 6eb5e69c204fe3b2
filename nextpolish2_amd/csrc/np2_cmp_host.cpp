// Host driver of the k-mer completeness join (np2_cmp.hip): np2_cmp_strings counts the assembly set into a table of its
// own that stays in HBM (the k-mer counter, np2_kcount_host.cpp), joins it with the reads' table in both directions and
// brings the spectrum and the counters back.  (np2_cmp.cpp would share the kernel file's object name.)
#include "np2_ctx.hpp"
#include "np2_cmp.hpp"
#include "np2_kcount.hpp"
#include "np2_kernel_timer.hpp"
#include "np2_pieces.hpp"

namespace {

// the grid: four blocks per CU (24 KiB of LDS each), striding over the table's turns; NP2_CMP_TEST_BLOCKS: a test's smaller
// grid, so that a small table takes several strides with an uneven last one
uint32_t cmp_blocks(int device) { return grid_blocks(device, 4, "NP2_CMP_TEST_BLOCKS"); }

} // namespace

extern "C" {

int np2_cmp_strings(np2_ctx_t *cx, int yak_idx, const uint8_t *strs, const uint64_t *off, uint64_t n, uint16_t min_count,
                    np2_cmp_t *out, uint64_t *spectra, uint64_t *asm_only, float *kernel_ms) {
    if (!cx) return NP2_E_ARG;
    return abi_guard([&] {
        // every argument is checked before anything is launched
        check_table(cx, yak_idx, "np2_cmp_strings", "yak_idx");
        if (min_count > np2kc::COUNT_MAX) throw Np2Error(NP2_E_ARG, "np2_cmp_strings: min_count must be at most 1023");
        if (!out) throw Np2Error(NP2_E_ARG, "np2_cmp_strings: out is NULL");
        check_string_set("np2_cmp_strings", strs, off, n);
        const YakTable &yt = cx->yaks[yak_idx];
        if (yt.ord)
            throw Np2Error(NP2_E_UNSUPPORTED, "np2_cmp_strings: table " + std::to_string(yak_idx) + " repeats keys: a k-mer would be "
                                              "counted once per word (distinct k-mers are what completeness is about)");
        *out = np2_cmp_t{0, 0, 0, 0};
        if (kernel_ms) *kernel_ms = 0.f;

        // the separator stream of the set: every sequence followed by one '\n', so that no k-mer spans two of them
        std::vector<uint8_t> stream;
        stream.reserve(n ? off[n] - off[0] + n : 0);
        for (uint64_t i = 0; i < n; ++i) {
            if (off[i + 1] > off[i]) stream.insert(stream.end(), strs + off[i], strs + off[i + 1]);
            stream.push_back('\n');
        }

        HIPCHK(hipSetDevice(cx->device));
        // cn(x): the counter's table with min_count 1, resident (one pass, or NP2_E_NOMEM), on this context's stream
        const np2h::ResidentCount ra = np2h::kcount_resident(cx->device, cx->stream, stream.data(), stream.size(), yt.k);

        DevBuf<uint64_t> d_out;
        d_out.cached = true; // (released after the read-back below)
        const size_t n_out = (size_t)CMP_SPECTRA + CMP_ASM_CTR;
        d_out.ensure(n_out);
        HIPCHK(hipMemsetAsync(d_out.p, 0, n_out * 8, cx->stream));
        const uint32_t blocks = cmp_blocks(cx->device), reliable = std::max<uint32_t>(min_count, 1u);
        KernelTimer timer(kernel_ms != nullptr);
        timer.start(cx->stream);
        // reliable read k-mers by their copy number in the set
        launch_cmp_join(cx->stream, CmpJoin{yt.table->p, ra.table->p, yt.cap_log2, ra.cap_log2, reliable, 1u,
                                            reinterpret_cast<unsigned long long *>(d_out.p)}, blocks);
        // the set's k-mers the reads do not have (a read count below min_count reads as 0: np2_qv_*'s rule)
        launch_cmp_asm_only(cx->stream, CmpJoin{ra.table->p, yt.table->p, ra.cap_log2, yt.cap_log2, 1u, reliable,
                                                reinterpret_cast<unsigned long long *>(d_out.p + CMP_SPECTRA)}, blocks);
        timer.stop(cx->stream);
        HIPCHK(hipGetLastError());
        std::vector<uint64_t> h(n_out);
        HIPCHK(hipMemcpyAsync(h.data(), d_out.p, n_out * 8, hipMemcpyDeviceToHost, cx->stream));
        HIPCHK(hipStreamSynchronize(cx->stream));
        timer.collect();

        // n_read and n_found are sums over the spectrum, not counters of their own
        for (uint32_t i = 0; i < CMP_SPECTRA; ++i) {
            out->n_read += h[i];
            if (i >= CMP_COUNTS) out->n_found += h[i];
        }
        out->n_asm = h[CMP_SPECTRA];
        for (uint32_t c = 0; c < CMP_CLASSES; ++c) out->n_asm_only += h[CMP_SPECTRA + 1 + c];
        if (spectra) memcpy(spectra, h.data(), (size_t)CMP_SPECTRA * 8);
        if (asm_only) memcpy(asm_only, h.data() + CMP_SPECTRA + 1, (size_t)CMP_CLASSES * 8);
        if (kernel_ms) *kernel_ms = timer.ms;
        return NP2_OK;
    }, ctx_sink(cx));
}

} // extern "C"

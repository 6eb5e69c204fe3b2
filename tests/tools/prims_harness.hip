// Test shim around the scan primitives libnp2_hip.so ships (tests/test_gpu_scan_prims.py).
//
// Host code only: every wrapper uploads the caller's host arrays whole (canaries and alignment padding included),
// calls the library's own np2::launch_* / np2::prim_* on device pointers at the caller's element offsets, synchronises
// and copies every array back.  A look-back launch gets a descriptor built here from the caller's ticket start, epoch
// and status pre-fill; the ticket counter starts at the ticket base, so the ticket accounting matches the grid.
// Returns 0, a hipError_t (> 0), or -1 when an offset / length does not fit the array it names (nothing is launched).
#include <cstdint>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../nextpolish2_amd/csrc/np2_kernels.hpp"

namespace {

struct Arr { // one host array mirrored on the device
    void *host;
    size_t bytes;
    char *dev;
};

struct Session {
    std::vector<Arr> arrs;
    hipStream_t s = nullptr;
    hipError_t e = hipSuccess;
    bool bad = false;
    Session() { e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    ~Session() {
        for (auto &a : arrs) (void)hipFree(a.dev);
        if (s) (void)hipStreamDestroy(s);
    }
    // device mirror of host[0 .. len) (elements of T), pointer to element off; need: elements from off the launch touches
    template <class T> T *up(T *host, uint64_t len, uint64_t off, uint64_t need) {
        if (e != hipSuccess || bad) return nullptr;
        if (!host || off > len || need > len - off) {
            bad = true;
            return nullptr;
        }
        Arr a{(void *)host, (size_t)len * sizeof(T), nullptr};
        e = hipMalloc((void **)&a.dev, a.bytes ? a.bytes : 16);
        if (e != hipSuccess) return nullptr;
        arrs.push_back(a);
        if (a.bytes) e = hipMemcpy(a.dev, host, a.bytes, hipMemcpyHostToDevice);
        return reinterpret_cast<T *>(a.dev) + off;
    }
    bool ready() const { return e == hipSuccess && !bad; }
    int finish() {
        if (bad) return -1;
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        for (auto &a : arrs)
            if (e == hipSuccess && a.bytes) e = hipMemcpy(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost);
        return (int)e;
    }
};

} // namespace

// Look-back descriptor of one launch: the status arrays (status[0 .. n_status) = a, [n_status, 2 n_status) = b) are
// uploaded as given and copied back; ticket[0] = the counter's start (= the descriptor's ticket base), and ticket[0]
// holds the counter after the launch on return; err: the device error word (in / out).
struct LbSpec {
    uint64_t *status;
    uint32_t n_status;
    uint32_t epoch;
    uint32_t *ticket;
    uint32_t *err;
};

static bool make_lb(Session &x, const LbSpec &sp, uint32_t n_blocks, np2::Lookback &lb, uint32_t *&err) {
    if (n_blocks > sp.n_status || sp.epoch == 0 || sp.epoch >= (1u << 30)) {
        x.bad = true;
        return false;
    }
    uint64_t *st = x.up(sp.status, 2ull * sp.n_status, 0, 2ull * sp.n_status);
    uint32_t *tk = x.up(sp.ticket, 1, 0, 1);
    err = x.up(sp.err, 1, 0, 1);
    if (!x.ready()) return false;
    lb = np2::Lookback{st, st + sp.n_status, tk, sp.ticket[0], sp.epoch, n_blocks, err};
    return true;
}

extern "C" {

uint32_t ph_scan_lb_blocks(uint64_t n) { return np2::scan_lb_blocks(n); }
uint32_t ph_tile_scan_blocks(uint32_t n_tiles) { return np2::tile_scan_blocks(n_tiles); }
uint32_t ph_cand_offsets_blocks(uint32_t n_reg) { return np2::cand_offsets_blocks(n_reg); }

// launch_scan_lb_excl (popc = 0: n elements, out[0 .. n + write_end)) or launch_scan_lb_popc (popc = 1: n words,
// out[0 .. n + 1))
int ph_scan_lb(int popc, uint32_t *in, uint64_t in_len, uint64_t in_off, uint32_t *out, uint64_t out_len, uint64_t out_off,
               uint32_t n, int write_end, const LbSpec *sp) {
    Session x;
    const uint32_t *din = x.up(in, in_len, in_off, n);
    uint32_t *dout = x.up(out, out_len, out_off, (uint64_t)n + (popc || write_end ? 1 : 0));
    np2::Lookback lb{};
    uint32_t *err = nullptr;
    if (x.ready() && make_lb(x, *sp, popc ? np2::scan_lb_blocks((uint64_t)n + 1) : np2::scan_lb_blocks(n), lb, err)) {
        if (popc)
            np2::launch_scan_lb_popc(x.s, lb, din, dout, n, err);
        else
            np2::launch_scan_lb_excl(x.s, lb, din, dout, n, write_end != 0, err);
    }
    return x.finish();
}

// mode 0: launch_scan_small_excl (total_out, write_end), 1: launch_scan_small_incl, 2: launch_scan_small_min.
// n_dev: nullptr, or the device-side count (one word); total: nullptr or one word.
int ph_scan_small(int mode, uint32_t *in, uint64_t in_len, uint32_t *out, uint64_t out_len, uint32_t n_host,
                  uint32_t *n_dev, uint32_t *total, int write_end) {
    Session x;
    const uint32_t *din = x.up(in, in_len, 0, n_host);
    uint32_t *dout = x.up(out, out_len, 0, (uint64_t)n_host + (write_end ? 1 : 0));
    const uint32_t *dn = n_dev ? x.up(n_dev, 1, 0, 1) : nullptr;
    uint32_t *dt = total ? x.up(total, 1, 0, 1) : nullptr;
    if (x.ready()) {
        if (mode == 0)
            np2::launch_scan_small_excl(x.s, din, dout, n_host, dn, dt, write_end != 0);
        else if (mode == 1)
            np2::launch_scan_small_incl(x.s, (const int32_t *)din, (int32_t *)dout, n_host, dn);
        else
            np2::launch_scan_small_min(x.s, (const int32_t *)din, (int32_t *)dout, n_host, dn);
    }
    return x.finish();
}

// mode 0: prim_exclusive_sum_u32, 1: prim_inclusive_sum_i32, 2: prim_inclusive_min_i32 (temporary storage sized by
// prim_temp_bytes); *status: the primitive's own return value
int ph_prim_scan(int mode, uint32_t *in, uint32_t *out, uint64_t n, int *status) {
    Session x;
    const uint32_t *din = x.up(in, n, 0, n);
    uint32_t *dout = x.up(out, n, 0, n);
    const size_t tb = np2::prim_temp_bytes(n);
    std::vector<uint8_t> tmp_host(tb, 0);
    void *tmp = x.up(tmp_host.data(), tb, 0, tb);
    if (x.ready()) {
        if (mode == 0)
            *status = np2::prim_exclusive_sum_u32(x.s, tmp, tb, din, dout, n);
        else if (mode == 1)
            *status = np2::prim_inclusive_sum_i32(x.s, tmp, tb, (const int32_t *)din, (int32_t *)dout, n);
        else
            *status = np2::prim_inclusive_min_i32(x.s, tmp, tb, (const int32_t *)din, (int32_t *)dout, n);
    }
    return x.finish();
}

// launch_tile_layout; tile_cur / tile_n: n_tiles + guard, tile_scan / tile_scanb: n_tiles + 1 + guard, out: 3 words.
// sp == nullptr: the one-block kernel, otherwise the look-back one.
int ph_tile_layout(uint32_t *tile_cur, uint32_t *tile_n, uint32_t *tile_scan, uint32_t *tile_scanb, uint64_t len,
                   uint32_t n_tiles, uint32_t bucket_cap, uint32_t *ovf_cnt, uint32_t *out, const LbSpec *sp) {
    Session x;
    uint32_t *dcur = x.up(tile_cur, len, 0, n_tiles), *dn = x.up(tile_n, len, 0, n_tiles);
    uint32_t *ds = x.up(tile_scan, len, 0, (uint64_t)n_tiles + 1), *dsb = x.up(tile_scanb, len, 0, (uint64_t)n_tiles + 1);
    const uint32_t *dovf = x.up(ovf_cnt, 1, 0, 1);
    uint32_t *dout = x.up(out, 3, 0, 3);
    np2::Lookback lb{};
    uint32_t *err = nullptr;
    if (x.ready() && (!sp || make_lb(x, *sp, np2::tile_scan_blocks(n_tiles), lb, err)))
        np2::launch_tile_layout(x.s, dcur, n_tiles, bucket_cap, dn, ds, dsb, dovf, dout, sp ? &lb : nullptr, err);
    return x.finish();
}

// launch_tile_offsets; tile_nn / tile_nr / tile_noff / tile_roff / tile_gain: len elements, reset: reset_len words
// (n_reset of them cleared), n_nodes / n_runs / gain_total: one word each; tile_gain == nullptr: no gain total
int ph_tile_offsets(uint32_t *tile_nn, uint32_t *tile_nr, uint32_t *tile_noff, uint32_t *tile_roff, uint64_t len,
                    uint32_t n_tiles, uint32_t *n_nodes, uint32_t *n_runs, uint32_t *reset, uint32_t reset_len,
                    uint32_t n_reset, int64_t *tile_gain, uint64_t *gain_total, const LbSpec *sp) {
    Session x;
    const uint32_t *dnn = x.up(tile_nn, len, 0, n_tiles), *dnr = x.up(tile_nr, len, 0, n_tiles);
    uint32_t *dno = x.up(tile_noff, len, 0, n_tiles), *dro = x.up(tile_roff, len, 0, n_tiles);
    uint32_t *dnodes = x.up(n_nodes, 1, 0, 1), *druns = x.up(n_runs, 1, 0, 1);
    uint32_t *dreset = x.up(reset, reset_len, 0, n_reset);
    const int64_t *dgain = tile_gain ? x.up(tile_gain, len, 0, n_tiles) : nullptr;
    uint64_t *dtot = tile_gain ? x.up(gain_total, 1, 0, 1) : nullptr;
    if (n_reset > (sp ? 256u : 1024u)) x.bad = true; // (one thread of the first block clears each word)
    np2::Lookback lb{};
    uint32_t *err = nullptr;
    if (x.ready() && (!sp || make_lb(x, *sp, np2::tile_scan_blocks(n_tiles), lb, err)))
        np2::launch_tile_offsets(x.s, dnn, dnr, n_tiles, dno, dro, dnodes, druns, dreset, n_reset, sp ? &lb : nullptr, err,
                                 (const long long *)dgain, (unsigned long long *)dtot);
    return x.finish();
}

// launch_cand_offsets; blk_sum: 3 n_blk words (n_blk = ceil(n_reg / 4)), blk_coff / blk_soff: blk_len elements,
// cand_off / reg_soff: reg_len elements (n_reg + 1 of them written), scal: n_cand, n_bytes, grow
int ph_cand_offsets(uint32_t *blk_sum, uint32_t *blk_coff, uint32_t *blk_soff, uint64_t blk_len, uint32_t *cand_off,
                    uint32_t *reg_soff, uint64_t reg_len, uint32_t n_reg, uint32_t *scal, const LbSpec *sp) {
    Session x;
    const uint64_t n_blk = ((uint64_t)n_reg + 3) / 4;
    const uint32_t *dsum = x.up(blk_sum, 3 * n_blk, 0, 3 * n_blk);
    uint32_t *dco = x.up(blk_coff, blk_len, 0, n_blk), *dso = x.up(blk_soff, blk_len, 0, n_blk);
    uint32_t *dcand = x.up(cand_off, reg_len, 0, (uint64_t)n_reg + 1), *dreg = x.up(reg_soff, reg_len, 0, (uint64_t)n_reg + 1);
    uint32_t *dscal = x.up(scal, 3, 0, 3);
    np2::Lookback lb{};
    uint32_t *err = nullptr;
    if (x.ready() && (!sp || make_lb(x, *sp, np2::cand_offsets_blocks(n_reg), lb, err)))
        np2::launch_cand_offsets(x.s, dsum, n_reg, dco, dso, dcand, dreg, dscal, dscal + 1, dscal + 2, sp ? &lb : nullptr, err);
    return x.finish();
}

} // extern "C"

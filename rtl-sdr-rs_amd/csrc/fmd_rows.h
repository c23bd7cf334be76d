// fmd_rows.h -- what the row processors share on the host: the handles that post-process the int16 rows a bank leaves on the device
// (fmd_resample.hip, fmd_agc.hip, fmd_tonesq.hip, fmd_dcs.hip, fmd_afsk.hip, fmd_fsk.hip) and the record banks that read such rows
// and leave records (fmd_hdlc.hip, fmd_pager.hip).  Their common contract: n_rows rows of `width` 1 or 2 int16 per sample, d_in
// [n_rows][in_cap][width] with n_in valid samples per row, d_out [n_rows][out_cap][width], a history pair of the samples in front
// of the call, core.pos counting input samples, and an output that does not depend on how the stream is cut.
// A handle embeds an FmdRows as its member `rows` and keeps its kernels, its launch struct, its own fields and domain checks, its
// counting function and the part of its enqueue that plans a call; where the handles differ they pass a callable.
// The record side (fmd_fsk.hip's hits, fmd_hdlc.hip, fmd_pager.hip): a call leaves [n_rows] counts and [n_rows][cap] fixed-size
// records on the device in an FmdRowRecords of the handle; behind the call the host reads the counts and min(count, cap) records of
// a row with zeros behind them.  The record banks have no d_out: their batch takes host rows and returns nothing.  Cumulative
// counters of the rows live in a `state` pair of the handle and are read by fmd_rows_read_state (fmd_tonesq.hip and fmd_dcs.hip
// read their status the same way); bytes a bank updates in place are an owned buffer of the core with a size and no source.
#pragma once

#include "fmd_ddc.h"

struct FmdRows {
    FmdDdcCore core;                                      // core.pos: input samples per row since creation or reset
    FmdDdcPair hist;                                      // [n_rows][hcap][width] int16: the samples in front of the next call
    uint32_t width = 0, n_rows = 0, hcap = 0;
    size_t lds = 0;                                       // dynamic LDS of a launch
};

// A *_new's first checks: the pointers (`arg` is the handle's own one), then the width.  Clears *out.
template <class H>
inline int fmd_rows_new_args(const void* arg, const fmd_device_config* dev, H** out, uint32_t width)
{
    if (!arg || !dev || !out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    if (width != 1 && width != 2) { fmd_internal_set_err("need width 1 or 2"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

// The row count, which both constructors check behind their own parameters.
inline int fmd_rows_count_arg(const fmd_device_config* dev)
{
    if (dev->n_channels < 1) { fmd_internal_set_err("need n_rows >= 1"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

// The end of a *_new, behind width, n_rows, hcap and lds: the history pair, the device step (an empty plan: the history and whatever
// else the handle registered are pairs and owned constants; 16 bytes of core history, which reset clears), then *out.  A failure
// deletes the handle or gives it to `free_h`.
template <class H, class Free>
inline int fmd_rows_device(H* h, const fmd_device_config* dev, Free free_h, H** out)
{
    FmdRows& r = h->rows;
    fmd_ddc_add_pair(r.core, r.hist, (size_t)r.n_rows * r.hcap * r.width * sizeof(int16_t));
    const char* what;
    if (const int rc = fmd_ddc_core_device(r.core, FmdDdcPlan(), 16, dev, &what)) {
        if (!what) { delete h; return rc; }
        fmd_internal_set_err(what); free_h(h); return rc;
    }
    *out = h;
    return FMD_OK;
}

// The checks every enqueue starts with.
inline int fmd_rows_check_call(const FmdRows& r, const void* d_in, size_t n_in, size_t in_cap, const void* d_out)
{
    const uintptr_t mask = 2u * r.width - 1u;
    if (((uintptr_t)d_in & mask) != 0 || ((uintptr_t)d_out & mask) != 0) { fmd_internal_set_err("misaligned device buffer"); return FMD_ERR_INVALID_ARG; }
    if (n_in > in_cap) { fmd_internal_set_err("n_in > in_cap"); return FMD_ERR_CAPACITY; }
    if (n_in > (1ull << 28)) { fmd_internal_set_err("n_in out of range"); return FMD_ERR_UNSUPPORTED; }
    return FMD_OK;
}

// The launch fields that describe the rows (same names in every launch struct); h and h_next, the history's lengths before and
// after the call, come from the handle's plan of the call.
template <class Launch>
inline void fmd_rows_fill(Launch& L, const FmdRows& r, const void* d_in, size_t n_in, size_t in_cap, void* d_out, size_t out_cap)
{
    L.in = static_cast<const int16_t*>(d_in); L.in_cap = in_cap; L.n_in = (uint32_t)n_in; L.n_rows = r.n_rows;
    L.hist_in = r.hist.in<int16_t>(r.core.cur); L.hist_out = r.hist.out<int16_t>(r.core.cur);
    L.hcap = r.hcap;
    L.out = static_cast<int16_t*>(d_out); L.out_cap = out_cap;
}

// The end of an enqueue: `k1` (width 1) or `k2` (width 2) over `grid` workgroups behind the stream order, the commit of n_in
// samples, the call's `cnt` outputs per row in *n_out.
template <class Launch>
inline int fmd_rows_launch(FmdRows& r, void (*k1)(const Launch), void (*k2)(const Launch), uint32_t grid, int threads, const Launch& L,
                           hipStream_t stream, size_t n_in, uint64_t cnt, size_t* n_out)
{
    FMD_DDC_TRY(r.core.order.before(stream));
    hipLaunchKernelGGL(r.width == 2 ? k2 : k1, dim3(grid), dim3(threads), r.lds, stream, L);
    FMD_DDC_TRY(hipGetLastError());
    fmd_ddc_commit(r.core, stream, n_in);
    if (n_out) *n_out = (size_t)cnt;
    return FMD_OK;
}

// The bodies of the entry points, over a handle H with the member `rows`.
template <class H>
inline void fmd_rows_free(H* h)
{
    if (!h) return;
    fmd_ddc_free(h->rows.core);
    delete h;
}

template <class H>
inline int fmd_rows_reset(H* h) { return h ? fmd_ddc_reset(h->rows.core) : FMD_ERR_INVALID_ARG; }

template <class H>
inline int fmd_rows_check(H* h)
{
    if (!h) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    return fmd_ddc_check(h->rows.core);
}

// `count(h, n)`: the outputs per row that exist once n samples per row have arrived.
template <class H, class Count>
inline int fmd_rows_outputs(const H* h, uint64_t* inputs, uint64_t* outputs, Count count)
{
    if (!h || !inputs || !outputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *inputs = h->rows.core.pos;
    *outputs = count(h, h->rows.core.pos);
    return FMD_OK;
}

// `fmt`: the kernel's name as rocprofv3 --kernel-trace prints it, with %u for the width.
template <class H>
inline int fmd_rows_kernel_name(const H* h, char* name, size_t cap, const char* fmt)
{
    if (!h || !name || cap == 0) return FMD_ERR_INVALID_ARG;
    return fmd_ddc_name_rc(snprintf(name, cap, fmt, h->rows.width), cap);
}

// (A `_run_device` entry point is fmd_ddc_run_device over the handle's enqueue, as the banks' are.)
// A `_run_batch` entry point: host in, host out, through the staging buffers on the handle's own stream, with the handle's
// enqueue(h, d_in, n_in, in_cap, d_out, out_cap, &n, stream).  `nothing(n_in)`: the handle has nothing to do for this call and says
// so before the device is touched (FMD_OK, no outputs).  A call that is accepted and emits nothing copies nothing back.
template <class H, class Enqueue, class Nothing>
inline int fmd_rows_run_batch(H* h, Enqueue enqueue, const int16_t* in, size_t n_in, size_t in_cap, int16_t* out, size_t out_cap,
                              size_t* n_out, Nothing nothing)
{
    if (!h || !in || !out || !n_out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (n_in > in_cap) { fmd_internal_set_err("n_in > in_cap"); return FMD_ERR_CAPACITY; }
    if (nothing(n_in)) { *n_out = 0; return FMD_OK; }
    FmdRows& r = h->rows;
    FmdDdcCore& c = r.core;
    FMD_DDC_ON_DEVICE(c.device);
    const size_t row = (size_t)r.width * sizeof(int16_t), in_bytes = r.n_rows * in_cap * row, out_bytes = r.n_rows * out_cap * row;
    FMD_DDC_TRY(fmd_ddc_grow(c.d_iq, c.d_iq_cap, in_bytes));
    FMD_DDC_TRY(fmd_ddc_grow(c.d_out, c.d_out_cap, out_bytes));
    FMD_DDC_TRY(hipMemcpyAsync(c.d_iq, in, in_bytes, hipMemcpyHostToDevice, c.stream));
    size_t n = 0;
    if (const int rc = enqueue(h, c.d_iq, n_in, in_cap, c.d_out, out_cap, &n, c.stream)) {
        (void)hipStreamSynchronize(c.stream);
        return rc;
    }
    if (n) FMD_DDC_TRY(hipMemcpyAsync(out, c.d_out, out_bytes, hipMemcpyDeviceToHost, c.stream));
    FMD_DDC_TRY(hipStreamSynchronize(c.stream));
    *n_out = n;
    return FMD_OK;
}

// ---- the record side ------------------------------------------------------------------------------------------------------------

// The results of a call: [n_rows] uint32 counts (up to a multiple of 16 bytes), then [n_rows][cap] records of rec_size bytes: written
// by a call, read behind it (the pair's other side is the call before).
struct FmdRowRecords {
    FmdDdcPair res;
    size_t rec_off = 0, rec_size = 0;                     // bytes of the counts in `res`, bytes of a record
    uint32_t cap = 0;                                     // records per row
    uint32_t* cnt_out(int cur) const { return res.out<uint32_t>(cur); }        // what the call that is being enqueued writes
    uint8_t* rec_out(int cur) const { return res.out<uint8_t>(cur) + rec_off; }
    const uint8_t* counts(int cur) const { return res.in<uint8_t>(cur); }      // what the last call wrote
    const uint8_t* records(int cur) const { return res.in<uint8_t>(cur) + rec_off; }
};

// bytes of [n_rows] counts in front of records that are read 16 bytes at a time
inline size_t fmd_rows_counts_bytes(size_t n_rows) { return (n_rows * sizeof(uint32_t) + 15u) & ~(size_t)15u; }

// In a *_new, behind n_rows: sizes the results and registers them on the core.
inline void fmd_rows_add_records(FmdRows& r, FmdRowRecords& q, uint32_t cap, size_t rec_size)
{
    q.cap = cap; q.rec_size = rec_size; q.rec_off = fmd_rows_counts_bytes(r.n_rows);
    fmd_ddc_add_pair(r.core, q.res, q.rec_off + (size_t)r.n_rows * cap * rec_size);
}

// the counts of the last call into cnt[n_rows], behind a device synchronisation (the caller holds the device guard)
inline int fmd_rows_read_counts(const FmdRows& r, const FmdRowRecords& q, uint32_t* cnt)
{
    FMD_DDC_TRY(hipDeviceSynchronize());
    FMD_DDC_TRY(hipMemcpy(cnt, q.counts(r.core.cur), r.n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return FMD_OK;
}

// behind the min(count, cap) records of a row at `dst`: zeros, not what an earlier call left.  Returns min(count, cap).
inline size_t fmd_rows_zero_behind(const FmdRowRecords& q, uint32_t count, void* dst)
{
    const size_t k = count < q.cap ? count : q.cap;
    memset(static_cast<uint8_t*>(dst) + k * q.rec_size, 0, (q.cap - k) * q.rec_size);
    return k;
}

// The bodies of a record bank's entry points, over a handle H with the members `rows` and `recs`.
template <class H>
inline int fmd_rows_inputs(const H* h, uint64_t* inputs)
{
    if (!h || !inputs) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *inputs = h->rows.core.pos;
    return FMD_OK;
}

template <class H>
inline int fmd_rows_counts(H* h, uint32_t* counts)
{
    if (!h || !counts) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(h->rows.core.device);
    return fmd_rows_read_counts(h->rows, h->recs, counts);
}

// The records of the listed rows into recs[n_sel][cap], in the order listed; nothing is touched before every argument has passed.
template <class H>
inline int fmd_rows_records(H* h, const uint32_t* rows, size_t n_sel, void* recs)
{
    if (!h || (n_sel && (!rows || !recs))) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    const FmdRows& r = h->rows;
    const FmdRowRecords& q = h->recs;
    for (size_t s = 0; s < n_sel; ++s)
        if (rows[s] >= r.n_rows) { fmd_internal_set_err("row out of range"); return FMD_ERR_INVALID_ARG; }
    FMD_DDC_ON_DEVICE(r.core.device);
    std::vector<uint32_t> cnt(r.n_rows);
    if (const int rc = fmd_rows_read_counts(r, q, cnt.data())) return rc;
    const size_t row_bytes = q.cap * q.rec_size;
    for (size_t s = 0; s < n_sel; ++s) {
        uint8_t* const dst = static_cast<uint8_t*>(recs) + s * row_bytes;
        const size_t k = fmd_rows_zero_behind(q, cnt[rows[s]], dst);
        if (k) FMD_DDC_TRY(hipMemcpy(dst, q.records(r.core.cur) + rows[s] * row_bytes, k * q.rec_size, hipMemcpyDeviceToHost));
    }
    return FMD_OK;
}

// The rows' carried state, `per_row` T each, as the last call left it: behind a device synchronisation, into `st`.
template <class T>
inline int fmd_rows_read_state(const FmdRows& r, const FmdDdcPair& state, size_t per_row, std::vector<T>& st)
{
    FMD_DDC_ON_DEVICE(r.core.device);
    FMD_DDC_TRY(hipDeviceSynchronize());
    st.resize(r.n_rows * per_row);
    FMD_DDC_TRY(hipMemcpy(st.data(), state.in<T>(r.core.cur), st.size() * sizeof(T), hipMemcpyDeviceToHost));
    return FMD_OK;
}

// A record bank's `_run_batch`: host rows in, nothing out -- the results stay on the device until they are asked for.  `more(core)`
// stages whatever the call reads beside the rows (a status other than FMD_OK ends the call), the rows go into core.d_iq, then
// enqueue(d_in, stream) on the handle's own stream.  A call of no samples does not touch the device.
template <class H, class More, class Enqueue>
inline int fmd_rows_feed_batch(H* h, const int16_t* in, size_t n_in, size_t in_cap, More more, Enqueue enqueue)
{
    if (!h || !in) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (n_in > in_cap) { fmd_internal_set_err("n_in > in_cap"); return FMD_ERR_CAPACITY; }
    if (n_in == 0) return FMD_OK;
    FmdDdcCore& c = h->rows.core;
    FMD_DDC_ON_DEVICE(c.device);
    const size_t in_bytes = (size_t)h->rows.n_rows * in_cap * sizeof(int16_t);
    FMD_DDC_TRY(fmd_ddc_grow(c.d_iq, c.d_iq_cap, in_bytes));
    if (const int rc = more(c)) return rc;
    FMD_DDC_TRY(hipMemcpyAsync(c.d_iq, in, in_bytes, hipMemcpyHostToDevice, c.stream));
    const int rc = enqueue(c.d_iq, c.stream);
    const hipError_t e = hipStreamSynchronize(c.stream);
    if (rc) return rc;                                       // (the enqueue's status wins over the synchronise's)
    FMD_DDC_TRY(e);
    return FMD_OK;
}

// ---- the pulse bank's results where they lie (fmd_pulses.hip), for the package bank that reads them there (fmd_packages.hip) --------

// What the pulse bank's last call that launched left on the device.  `order` is the bank's own: a reader on another stream waits
// behind it.  The pointers hold until the bank's next call but one.
struct FmdPulsesLast {
    int device = 0;
    uint32_t n_streams = 0, pulse_cap = 0;
    bool launched = false;                                // since creation or reset
    uint32_t n_samples = 0;                               // per stream, of that call
    const uint32_t* d_counts = nullptr;                   // [n_streams]
    const uint8_t* d_recs = nullptr;                      // [n_streams][pulse_cap] fmd_pulses_rec
    const uint32_t* d_state = nullptr;                    // [n_streams][state_dwords]: samples (u64) at dword 0, the run (u64) at 6, s at 8
    uint32_t state_dwords = 0;
    FmdStreamOrder* order = nullptr;
};
void fmd_pulses_last(fmd_pulses* h, FmdPulsesLast* out);

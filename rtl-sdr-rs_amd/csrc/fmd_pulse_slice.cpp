// fmd_pulse_slice.cpp -- the host slicer behind the pulse bank (include/fmd.h, fmd_pulse_slicer_*): the pulse records of one stream
// in, PWM / PPM bit packages out.  Host only, fixed buffers, nothing of the library but the header.  Definition:
// tests/pulse_slice_ref.py.
#include "../../include/fmd.h"

#include <cstring>
#include <new>

void fmd_internal_set_err(const char* msg);

namespace {
constexpr size_t kWaiting = 64;                          // closed packages that wait for _take
constexpr uint32_t kMaxBits = 256;
}

struct fmd_pulse_slicer {
    fmd_pulse_slicer_config cfg{};
    bool open = false;
    fmd_pulse_package cur{};                              // the open package
    fmd_pulse_package ring[kWaiting];
    size_t head = 0, count = 0;                           // the oldest waiting package, how many wait
};

namespace {

void close_package(fmd_pulse_slicer* p)
{
    if (p->count < kWaiting) p->ring[(p->head + p->count++) % kWaiting] = p->cur;    // (else it is dropped)
    p->open = false;
}

bool near(uint32_t v, uint32_t centre, uint32_t tol) { return (v > centre ? v - centre : centre - v) <= tol; }

void take_pulse(fmd_pulse_slicer* p, const fmd_pulses_rec& r, uint64_t pos)
{
    const fmd_pulse_slicer_config& c = p->cfg;
    if (p->open && r.gap >= c.reset) close_package(p);
    const bool first = !p->open;
    if (first) {
        const uint64_t fall = pos + (uint64_t)(int64_t)r.k_rel;
        memset(&p->cur, 0, sizeof p->cur);
        p->cur.start = fall >= r.width ? fall - r.width : 0;
        p->open = true;
    }
    fmd_pulse_package& k = p->cur;
    if (k.n_pulses != 0xFFFFFFFFu) ++k.n_pulses;
    if (k.flags & FMD_PULSE_BAD) return;                     // skip to the package's end
    uint32_t bit;
    if (c.modulation == FMD_PULSE_PWM) {
        if (near(r.width, c.short_w, c.tol)) bit = 1u;
        else if (near(r.width, c.long_w, c.tol)) bit = 0u;
        else { k.flags |= FMD_PULSE_BAD; return; }
    } else {
        if (first) return;                                   // the first pulse only opens the package
        if (near(r.gap, c.short_w, c.tol)) bit = 0u;
        else if (near(r.gap, c.long_w, c.tol)) bit = 1u;
        else { k.flags |= FMD_PULSE_BAD; return; }
    }
    if (k.n_bits == kMaxBits) { k.flags |= FMD_PULSE_TRUNCATED; return; }
    if (bit) k.bits[k.n_bits >> 3] |= (uint8_t)(0x80u >> (k.n_bits & 7u));
    ++k.n_bits;
}

}  // namespace

extern "C" {

int fmd_pulse_slicer_new(const fmd_pulse_slicer_config* cfg, fmd_pulse_slicer** out)
{
    if (!cfg || !out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    *out = nullptr;
    if (cfg->modulation > FMD_PULSE_PPM) { fmd_internal_set_err("need modulation 0 (PWM) or 1 (PPM)"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->short_w < 1u || cfg->long_w < 1u) { fmd_internal_set_err("need short_w and long_w >= 1"); return FMD_ERR_UNSUPPORTED; }
    if (cfg->reset < 1u) { fmd_internal_set_err("need reset >= 1"); return FMD_ERR_UNSUPPORTED; }
    fmd_pulse_slicer* p = new (std::nothrow) fmd_pulse_slicer();
    if (!p) return FMD_ERR_NOMEM;
    p->cfg = *cfg;
    *out = p;
    return FMD_OK;
}

void fmd_pulse_slicer_free(fmd_pulse_slicer* p) { delete p; }

int fmd_pulse_slicer_push(fmd_pulse_slicer* p, const fmd_pulses_rec* recs, size_t n, uint64_t pos)
{
    if (!p || (n && !recs)) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    for (size_t i = 0; i < n; ++i) take_pulse(p, recs[i], pos);
    return FMD_OK;
}

int fmd_pulse_slicer_idle(fmd_pulse_slicer* p, uint32_t state, uint64_t run)
{
    if (!p) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (p->open && state == 0u && run >= p->cfg.reset) close_package(p);
    return FMD_OK;
}

int fmd_pulse_slicer_take(fmd_pulse_slicer* p, fmd_pulse_package* packages, size_t cap, size_t* n)
{
    if (!p || !n || (cap && !packages)) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    const size_t k = p->count < cap ? p->count : cap;
    for (size_t i = 0; i < k; ++i) packages[i] = p->ring[(p->head + i) % kWaiting];
    p->head = (p->head + k) % kWaiting;
    p->count -= k;
    *n = k;
    return FMD_OK;
}

}  // extern "C"

// fmd_modes_decode.cpp -- the host side of the Mode S bank (include/fmd.h, "Mode S bank"): the syndrome table and the syndrome of a
// message as the kernel forms them, and what an extended squitter says -- address, type code, callsign, barometric altitude,
// velocity, the CPR pair -- with the global CPR solve.  Host only: nothing here touches a device.
#include "../../include/fmd.h"

#include <cmath>
#include <cstring>

void fmd_internal_set_err(const char* msg);

namespace {

constexpr uint32_t kGenerator = 0xFFF409u;

// T_112[t] = x^(111 - t) mod the generator (x^24 + the 24 bits of kGenerator)
void ms_table112(uint32_t* t112)
{
    uint32_t v = 1u;
    for (int t = 111; t >= 0; --t) {
        t112[t] = v;
        v = (v & 0x800000u) ? ((v << 1) & 0xFFFFFFu) ^ kGenerator : v << 1;
    }
}

uint32_t ms_bits(const uint8_t* b, uint32_t first, uint32_t len)
{
    uint32_t v = 0;
    for (uint32_t i = first; i < first + len; ++i) v = v << 1 | ((b[i >> 3] >> (7u - (i & 7u))) & 1u);
    return v;
}

// the number of longitude zones at a latitude (NZ = 15)
int ms_nl(double lat)
{
    const double pi = 3.14159265358979323846;
    lat = std::fabs(lat);
    if (lat < 1e-9) return 59;
    if (lat > 87.0) return 1;
    if (lat == 87.0) return 2;
    const double c = std::cos(pi / 180.0 * lat);
    return (int)std::floor(2.0 * pi / std::acos(1.0 - (1.0 - std::cos(pi / 30.0)) / (c * c)));
}

double ms_mod(double a, double b) { return a - b * std::floor(a / b); }

}  // namespace

extern "C" {

int fmd_modes_table(uint32_t n_bits, uint32_t* table)
{
    if (!table) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (n_bits != 56 && n_bits != 112) { fmd_internal_set_err("need n_bits 56 or 112"); return FMD_ERR_UNSUPPORTED; }
    uint32_t t112[112];
    ms_table112(t112);
    memcpy(table, t112 + (112 - n_bits), n_bits * sizeof(uint32_t));
    return FMD_OK;
}

int fmd_modes_syndrome(const uint8_t* bytes, size_t n_bytes, uint32_t* syn)
{
    if (!bytes || !syn) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if (n_bytes != 7 && n_bytes != 14) { fmd_internal_set_err("need n_bytes 7 or 14"); return FMD_ERR_BAD_LENGTH; }
    uint32_t t112[112];
    ms_table112(t112);
    const uint32_t n = 8u * (uint32_t)n_bytes;
    uint32_t s = 0;
    for (uint32_t t = 0; t < n; ++t)
        if (ms_bits(bytes, t, 1)) s ^= t112[t + 112u - n];
    *syn = s;
    return FMD_OK;
}

int fmd_modes_decode(const uint8_t* bytes, size_t n_bytes, fmd_modes_fields* out)
{
    if (!bytes || !out) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    if (n_bytes != 14 || ((bytes[0] >> 3) != 17 && (bytes[0] >> 3) != 18)) {
        fmd_internal_set_err("need an extended squitter: 14 bytes, DF 17 or 18");
        return FMD_ERR_UNSUPPORTED;
    }
    out->df = bytes[0] >> 3;
    out->icao = ms_bits(bytes, 8, 24);
    const uint32_t tc = ms_bits(bytes, 32, 5);
    out->type_code = tc;
    out->subtype = ms_bits(bytes, 37, 3);
    if (tc >= 1 && tc <= 4) {
        static const char kSet[] = "#ABCDEFGHIJKLMNOPQRSTUVWXYZ##### ###############0123456789######";
        for (uint32_t i = 0; i < 8; ++i) out->callsign[i] = kSet[ms_bits(bytes, 40 + 6 * i, 6)];
        for (int i = 7; i >= 0 && out->callsign[i] == ' '; --i) out->callsign[i] = 0;
        out->has |= 1u;
    } else if (tc >= 9 && tc <= 18) {
        if (ms_bits(bytes, 47, 1)) {                         // the Q bit: 25 ft steps
            const uint32_t n = ms_bits(bytes, 40, 7) << 4 | ms_bits(bytes, 48, 4);
            out->altitude_ft = (int32_t)(25u * n) - 1000;
            out->has |= 2u;
        }
        out->cpr_odd = ms_bits(bytes, 53, 1);
        out->cpr_lat = ms_bits(bytes, 54, 17);
        out->cpr_lon = ms_bits(bytes, 71, 17);
        out->has |= 4u;
    } else if (tc == 19 && (out->subtype == 1 || out->subtype == 2)) {
        const uint32_t vew = ms_bits(bytes, 46, 10), vns = ms_bits(bytes, 57, 10), vr = ms_bits(bytes, 69, 9);
        if (vew && vns && vr) {                              // 0: not available
            const int scale = out->subtype == 2 ? 4 : 1;
            const int vx = (ms_bits(bytes, 45, 1) ? -1 : 1) * scale * (int)(vew - 1);     // east
            const int vy = (ms_bits(bytes, 56, 1) ? -1 : 1) * scale * (int)(vns - 1);     // north
            out->speed_kt = std::sqrt((double)(vx * vx + vy * vy));
            double trk = std::atan2((double)vx, (double)vy) * (180.0 / 3.14159265358979323846);
            if (trk < 0) trk += 360.0;
            out->track_deg = trk;
            out->vrate_fpm = (ms_bits(bytes, 68, 1) ? -1 : 1) * 64 * (int)(vr - 1);
            out->has |= 8u;
        }
    }
    return FMD_OK;
}

int fmd_modes_cpr_global(uint32_t lat_even, uint32_t lon_even, uint32_t lat_odd, uint32_t lon_odd, int latest_odd, double* lat, double* lon)
{
    if (!lat || !lon) { fmd_internal_set_err("null argument"); return FMD_ERR_INVALID_ARG; }
    if ((lat_even | lon_even | lat_odd | lon_odd) >> 17) { fmd_internal_set_err("need 17-bit CPR values"); return FMD_ERR_UNSUPPORTED; }
    const double le = lat_even / 131072.0, lo = lat_odd / 131072.0, ge = lon_even / 131072.0, go = lon_odd / 131072.0;
    const double j = std::floor(59.0 * le - 60.0 * lo + 0.5);
    double re = 6.0 * (ms_mod(j, 60.0) + le), ro = (360.0 / 59.0) * (ms_mod(j, 59.0) + lo);
    if (re >= 270.0) re -= 360.0;
    if (ro >= 270.0) ro -= 360.0;
    if (re < -90.0 || re > 90.0 || ro < -90.0 || ro > 90.0) { fmd_internal_set_err("the pair gives no latitude"); return FMD_ERR_BAD_STATE; }
    if (ms_nl(re) != ms_nl(ro)) { fmd_internal_set_err("the pair straddles a longitude zone boundary"); return FMD_ERR_BAD_STATE; }
    const int nl = ms_nl(latest_odd ? ro : re);
    const int ni = latest_odd ? (nl - 1 > 1 ? nl - 1 : 1) : (nl > 1 ? nl : 1);
    const double m = std::floor(ge * (nl - 1) - go * nl + 0.5);
    double g = (360.0 / ni) * (ms_mod(m, (double)ni) + (latest_odd ? go : ge));
    if (g >= 180.0) g -= 360.0;
    *lat = latest_odd ? ro : re;
    *lon = g;
    return FMD_OK;
}

}  // extern "C"

// emu_robust.cpp — TEST TOOL: vk_robust_resolve's per-pixel arithmetic on the host.  The ordering, G, the trim, the kept sums and the
// standard error are the kernel's own — vk_robust.h robust_resolve_pixel<K>, built here with g++, one instance per K as the device
// builds them.  Built into tests/emu's library only.
#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_robust.h"

static thread_local std::string g_robust_err;

namespace {

template <int K>
void resolve_tables(const long long *tables, uint64_t n, uint32_t mode, uint32_t trim, float *rgb, float *se) {
    for (uint64_t p = 0; p < n; p++) {
        RobustCell tab[K];                               // (the caller's memory need not be aligned as the device's is)
        for (int b = 0; b < K; b++)
            for (int c = 0; c < 4; c++) tab[b].v[c] = tables[(p * K + b) * 4u + c];
        robust_resolve_pixel<K>(tab, mode, trim, rgb + p * 3u, se + p * 3u);
    }
}

}  // namespace

extern "C" {

const char *emu_robust_last_error() { return g_robust_err.c_str(); }

// tables: n * buckets * 4 values, [(pixel * buckets + b) * 4 + c] as vk_debug_robust_sums gives them; rgb, se: n * 3 floats each
int emu_robust_resolve(uint32_t buckets, const long long *tables, uint64_t n, uint32_t mode, uint32_t trim, float *rgb, float *se) {
    if (!tables || !rgb || !se) { g_robust_err = "null argument"; return VK_ERR_BAD_ARG; }
    if (mode > (uint32_t)VK_ROBUST_GINI) { g_robust_err = "unknown mode"; return VK_ERR_BAD_ARG; }
    switch (buckets) {
        case 2: resolve_tables<2>(tables, n, mode, trim, rgb, se); break;
        case 3: resolve_tables<3>(tables, n, mode, trim, rgb, se); break;
        case 4: resolve_tables<4>(tables, n, mode, trim, rgb, se); break;
        case 5: resolve_tables<5>(tables, n, mode, trim, rgb, se); break;
        case 6: resolve_tables<6>(tables, n, mode, trim, rgb, se); break;
        case 7: resolve_tables<7>(tables, n, mode, trim, rgb, se); break;
        case 8: resolve_tables<8>(tables, n, mode, trim, rgb, se); break;
        case 9: resolve_tables<9>(tables, n, mode, trim, rgb, se); break;
        case 10: resolve_tables<10>(tables, n, mode, trim, rgb, se); break;
        case 11: resolve_tables<11>(tables, n, mode, trim, rgb, se); break;
        case 12: resolve_tables<12>(tables, n, mode, trim, rgb, se); break;
        case 13: resolve_tables<13>(tables, n, mode, trim, rgb, se); break;
        case 14: resolve_tables<14>(tables, n, mode, trim, rgb, se); break;
        case 15: resolve_tables<15>(tables, n, mode, trim, rgb, se); break;
        case 16: resolve_tables<16>(tables, n, mode, trim, rgb, se); break;
        default: g_robust_err = "buckets must be in 2..16"; return VK_ERR_BAD_ARG;
    }
    return VK_OK;
}

}  // extern "C"

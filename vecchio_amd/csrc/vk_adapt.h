// vk_adapt.h — the kernels of vk_adapt.hip as vk_api.hip sees them: their argument records and one thin launcher each
// (launch_adapt_*(args), on the null stream of the current device; the caller checks hipGetLastError).  The index code of a tile run,
// adapt_locate, is host-and-device: tests/emu/emu_adapt.cpp builds it with g++.
#ifndef VK_ADAPT_H
#define VK_ADAPT_H

#include <stdint.h>

#include "vk_math.h"        // VK_HD

// The active tiles of a film as a tile run sees them: list[a] = the a-th active tile (ascending tile index t = ty * tiles_x + tx, tile
// row 0 at the bottom), prefix[a] = P_a, the in-image pixels of the active tiles before it (prefix[n_active] = all of them).  With width
// and height multiples of 8 every tile has 64 pixels: whole = 1 and prefix is not read.
struct AdaptTiles {
    const uint32_t *list;
    const uint32_t *prefix;
    uint32_t n_active, width, height, tiles_x, whole;
};

// Path q of a tile run of n_samples samples over T: p = q / n_samples, k = q - p * n_samples, a = the largest index with P_a <= p,
// j = p - P_a; pixel j of tile list[a] is x = 8 tx + j % tw, y = 8 ty + j / tw with tw = min(8, width - 8 tx), th likewise.  Returns the
// pixel's row-major index y * width + x; q < P_{n_active} * n_samples is the caller's to ensure.
VK_HD uint32_t adapt_locate(const AdaptTiles &T, uint32_t n_samples, uint32_t q, uint32_t &x, uint32_t &y, uint32_t &k) {
    const uint32_t p = q / n_samples;
    k = q - p * n_samples;
    uint32_t a, j;
    if (T.whole) {
        a = p >> 6; j = p & 63u;
    } else {
        uint32_t lo = 0u, hi = T.n_active;       // P_lo <= p < P_hi
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (T.prefix[mid] <= p) lo = mid; else hi = mid;
        }
        a = lo; j = p - T.prefix[a];
    }
    const uint32_t t = T.list[a];
    const uint32_t ty = t / T.tiles_x, tx = t - ty * T.tiles_x;
    const uint32_t left = T.width - 8u * tx, tw = left < 8u ? left : 8u;
    const uint32_t jy = j / tw;
    x = 8u * tx + (j - jy * tw); y = 8u * ty + jy;
    return y * T.width + x;
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

#include "vk_trace.h"       // RenderConsts

// adapt_emit_kernel, the top-up of a tile run: lane j < m starts path first + j of the run in slot slot0 + j, id = its number
struct AdaptEmitArgs {
    vkd::RenderConsts C;     // the film's camera, frame and seed
    uint4 *rays;             // vk_ray[capacity]
    uint4 *states;           // vk_path_state[capacity]
    uint32_t *ids;           // [capacity]: the buffer that holds the live ids of this bounce
    AdaptTiles T;
    uint32_t first_sample, n_samples;
    uint32_t first, slot0, m;
};
// adapt_sequence_kernel (vk_debug_adapt_sequence): the same index code, its answers stored instead of started
struct AdaptSequenceArgs {
    AdaptTiles T;
    uint32_t first_sample, n_samples, first, m;
    uint32_t *pixel_out, *sample_out;      // [m]
};
// adapt_close_kernel: fold and judge, one wave per active tile
struct AdaptCloseArgs {
    const long long *sums;   // the film's
    long long *prev;
    double *m2;
    const uint32_t *list;
    uint32_t *tile_n, *tile_k;
    uint32_t n_active, width, height, tiles_x;
    uint32_t window, done, steps, gate;    // this close's n_samples; samples_done and steps behind it; gate = the rule may freeze now
    float abs_tol, rel_tol;
};
// adapt_count_kernel and adapt_scatter_kernel: the list and its pixel prefix from the tile map
struct AdaptListArgs {
    const uint32_t *tile_n;
    uint32_t *list, *prefix;
    uint32_t *block_tiles, *block_px;      // [ceil(tiles / 1024)] each
    unsigned long long *record;            // [2]: the active tiles, their in-image pixels
    uint32_t tiles, width, height, tiles_x;
};
// adapt_resolve_kernel and adapt_stderr_kernel: one lane per pixel, from the sums of the last close
struct AdaptImageArgs {
    const long long *prev;
    const double *m2;        // (the resolve reads none)
    const uint32_t *tile_n, *tile_k;
    float *out;
    uint32_t width, height, tiles_x, done, steps;
};

void launch_adapt_emit(const AdaptEmitArgs &A);
void launch_adapt_sequence(const AdaptSequenceArgs &A);
void launch_adapt_close(const AdaptCloseArgs &A);
void launch_adapt_list(const AdaptListArgs &A);          // two launches
void launch_adapt_resolve(const AdaptImageArgs &A);
void launch_adapt_stderr(const AdaptImageArgs &A);
#endif

#endif

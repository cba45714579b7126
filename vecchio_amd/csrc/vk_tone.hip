// vk_tone.hip — the kernels behind vk_tone_* (include/vecchio_amd.h "display transform"): a frame's luminance histogram and its encoding
// to 8-bit display codes.  A translation unit of its own (vk_kernels.h belongs to vk_api.hip): the C ABI, the handle, the exposure's host
// half and the argument checks stay in vk_api.hip, which calls the launchers at the end of this file.
//
// Everything a kernel adds up is an integer: the histogram and the counters do not depend on the launch shape or the form.  The
// per-pixel code is vk_tone.h's, shared with the host build of tests/emu.
#include <hip/hip_runtime.h>

#include "vk_tone.h"

namespace {

constexpr int TONE_T = 256;                            // 4 waves a workgroup
// the LDS form's grid: one workgroup a CU.  Every workgroup ends on up to 640 global atomics on the same 640 words, and those — not the
// frame's bytes — were what a grid of 1024 workgroups waited for (DESIGN.md "Display transform")
constexpr uint32_t TONE_METER_MAX_BLOCKS = 256u;

// the wave's sum of v in lane 0
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// the four counters of a wave's lanes: one atomic per wave and non-zero counter.  Every lane of the wave calls it.
__device__ __forceinline__ void tone_count_wave(unsigned long long *counters, const uint32_t n[4]) {
    for (uint32_t k = 0; k < TONE_COUNTERS; k++) {
        const uint32_t s = wave_sum(n[k]);
        if ((threadIdx.x & 63u) == 0u && s != 0u) atomicAdd(counters + k, (unsigned long long)s);
    }
}

}  // namespace

// tone_meter_lds_kernel: a workgroup-private histogram in LDS (2560 bytes), a grid-stride loop over groups of four pixels — 48 bytes, three
// 16-byte loads a lane — and behind it over the frame's last n % 4 pixels, LDS integer atomics, and at the end one global atomic per
// non-zero bin of the workgroup.  A lane adds each run of equal bins among its four pixels at once (neighbours mostly share a bin), and
// a wave whose lanes all hold one run of one bin (a flat frame: 64 lanes on one LDS address) adds its count through one lane.  The
// four counters are kept per lane and reduced across the wave before one atomic each.
__global__ __launch_bounds__(TONE_T) void tone_meter_lds_kernel(ToneMeterArgs A) {
    __shared__ uint32_t hist[TONE_BINS];
    for (uint32_t b = threadIdx.x; b < TONE_BINS; b += TONE_T) hist[b] = 0u;
    __syncthreads();
    uint32_t n[4] = {0u, 0u, 0u, 0u};
    const uint32_t groups = A.n_pixels / 4u, stride = gridDim.x * TONE_T;
    const float4 *in = reinterpret_cast<const float4 *>(A.rgb);
    for (uint32_t g = blockIdx.x * TONE_T + threadIdx.x; g < groups; g += stride) {
        const float4 a = in[(size_t)g * 3u], b = in[(size_t)g * 3u + 1u], c = in[(size_t)g * 3u + 2u];
        const uint32_t w[4] = {tone_classify(a.x, a.y, a.z), tone_classify(a.w, b.x, b.y), tone_classify(b.z, b.w, c.x),
                               tone_classify(c.y, c.z, c.w)};
        // the wave's shortcut: every active lane holds four pixels of the first lane's bin
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)w[0]);
        const unsigned long long active = __ballot(1);
        const unsigned long long same = __ballot(w[0] == first && w[1] == first && w[2] == first && w[3] == first);
        if (same == active && first < TONE_BINS) {
            if ((threadIdx.x & 63u) == (uint32_t)__ffsll((long long)active) - 1u) atomicAdd(&hist[first], 4u * (uint32_t)__popcll(active));
            n[TONE_BINNED] += 4u;
            continue;
        }
        // otherwise the lane's own runs of equal values: one add per run
        uint32_t cur = w[0], run = 1u;
        for (int k = 1; k <= 4; k++) {
            if (k < 4 && w[k] == cur) { run++; continue; }
            if (cur < TONE_BINS) { atomicAdd(&hist[cur], run); n[TONE_BINNED] += run; }
            else n[cur - TONE_BINS] += run;
            if (k < 4) { cur = w[k]; run = 1u; }
        }
    }
    // the tail: pixels 4 * groups .. n_pixels - 1, by the first lanes of workgroup 0
    const uint32_t tail = groups * 4u + threadIdx.x;
    if (blockIdx.x == 0u && threadIdx.x < 4u && tail < A.n_pixels) {
        const float *q = A.rgb + (size_t)tail * 3u;
        const uint32_t w = tone_classify(q[0], q[1], q[2]);
        if (w < TONE_BINS) { atomicAdd(&hist[w], 1u); n[TONE_BINNED] += 1u; }
        else n[w - TONE_BINS] += 1u;
    }
    tone_count_wave(A.counters, n);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < TONE_BINS; b += TONE_T) {
        const uint32_t v = hist[b];
        if (v != 0u) atomicAdd(A.bins + b, v);
    }
}

// tone_meter_plain_kernel: one lane per pixel, one global atomic per binned pixel (the PLAIN form, kept for A/B); the counters as above
__global__ __launch_bounds__(TONE_T) void tone_meter_plain_kernel(ToneMeterArgs A) {
    const uint32_t i = blockIdx.x * TONE_T + threadIdx.x;
    uint32_t n[4] = {0u, 0u, 0u, 0u};
    if (i < A.n_pixels) {
        const float *q = A.rgb + (size_t)i * 3u;
        const uint32_t w = tone_classify(q[0], q[1], q[2]);
        if (w < TONE_BINS) { atomicAdd(A.bins + w, 1u); n[TONE_BINNED] = 1u; }
        else n[w - TONE_BINS] = 1u;
    }
    tone_count_wave(A.counters, n);
}

// tone_encode_kernel<CURVE, TABLE, DITHER>: one lane per four consecutive OUTPUT pixels (row 0 the top) — twelve bytes, three dword
// stores; the image's last n % 4 pixels leave as bytes.  A group that lies in one row and starts on a multiple of four input pixels is
// read with three 16-byte loads (every group of a frame whose width is a multiple of 4); any other group — one that straddles a row
// end among them — pixel by pixel.  The table instances stage the 510 thresholds in LDS (2040 bytes) first.
template <uint32_t CURVE, bool TABLE, bool DITHER>
__global__ __launch_bounds__(TONE_T) void tone_encode_kernel(ToneEncodeArgs A) {
    const float *h = nullptr;
    if constexpr (TABLE) {
        __shared__ float staged[TONE_TABLE];
        for (uint32_t j = threadIdx.x; j < TONE_TABLE; j += TONE_T) staged[j] = A.table[j];
        __syncthreads();
        h = staged;
    }
    const uint32_t n = A.width * A.height;
    const uint32_t o0 = (blockIdx.x * TONE_T + threadIdx.x) * 4u;
    if (o0 >= n) return;
    const uint32_t count = n - o0 < 4u ? n - o0 : 4u;
    const uint32_t row0 = o0 / A.width, x0 = o0 - row0 * A.width;
    const uint32_t in0 = (A.height - 1u - row0) * A.width + x0;
    float v[12];
    uint32_t pix[4];
    if (count == 4u && x0 + 4u <= A.width && (in0 & 3u) == 0u) {
        const float4 *in = reinterpret_cast<const float4 *>(A.rgb + (size_t)in0 * 3u);
        const float4 a = in[0], b = in[1], c = in[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
        for (uint32_t k = 0; k < 4u; k++) pix[k] = in0 + k;
    } else {
        uint32_t row = row0, x = x0;
        for (uint32_t k = 0; k < 4u; k++) {
            const bool live = k < count;
            pix[k] = live ? (A.height - 1u - row) * A.width + x : 0u;
            const float *q = A.rgb + (size_t)pix[k] * 3u;
            v[3u * k] = live ? q[0] : 0.0f; v[3u * k + 1u] = live ? q[1] : 0.0f; v[3u * k + 2u] = live ? q[2] : 0.0f;
            if (++x == A.width) { x = 0u; row++; }
        }
    }
    uint32_t code[12];
    for (uint32_t k = 0; k < 4u; k++) tone_pixel<CURVE, TABLE, DITHER>(v + 3u * k, h, A.E, A.p, A.seed, pix[k], code + 3u * k);
    uint8_t *out = A.out + (size_t)o0 * 3u;
    if (count == 4u) {
        uint32_t *o = reinterpret_cast<uint32_t *>(out);
        o[0] = code[0] | code[1] << 8 | code[2] << 16 | code[3] << 24;
        o[1] = code[4] | code[5] << 8 | code[6] << 16 | code[7] << 24;
        o[2] = code[8] | code[9] << 8 | code[10] << 16 | code[11] << 24;
    } else {
        for (uint32_t k = 0; k < 4u; k++) {
            if (k < count) { out[3u * k] = (uint8_t)code[3u * k]; out[3u * k + 1u] = (uint8_t)code[3u * k + 1u]; out[3u * k + 2u] = (uint8_t)code[3u * k + 2u]; }
        }
    }
}

// ---- the launchers (vk_tone.h): null stream, current device; sizes > 0 are the caller's to ensure
void launch_tone_meter(const ToneMeterArgs &A, uint32_t form) {
    if (form == TONE_FORM_PLAIN) {
        hipLaunchKernelGGL(tone_meter_plain_kernel, dim3((A.n_pixels + TONE_T - 1) / TONE_T), dim3(TONE_T), 0, nullptr, A);
    } else {
        const uint32_t groups = A.n_pixels / 4u, want = (groups + TONE_T - 1) / TONE_T;
        const uint32_t blocks = want < 1u ? 1u : (want > TONE_METER_MAX_BLOCKS ? TONE_METER_MAX_BLOCKS : want);
        hipLaunchKernelGGL(tone_meter_lds_kernel, dim3(blocks), dim3(TONE_T), 0, nullptr, A);
    }
}

namespace {

template <uint32_t CURVE>
void launch_encode_curve(const ToneEncodeArgs &A, bool table, bool dither) {
    const uint32_t groups = (A.width * A.height + 3u) / 4u;
    const dim3 grid((groups + TONE_T - 1) / TONE_T), block(TONE_T);
    if (!table) hipLaunchKernelGGL((tone_encode_kernel<CURVE, false, false>), grid, block, 0, nullptr, A);
    else if (!dither) hipLaunchKernelGGL((tone_encode_kernel<CURVE, true, false>), grid, block, 0, nullptr, A);
    else hipLaunchKernelGGL((tone_encode_kernel<CURVE, true, true>), grid, block, 0, nullptr, A);
}

}  // namespace

void launch_tone_encode(const ToneEncodeArgs &A, uint32_t curve, bool table, bool dither) {
    switch (curve) {
        case TONE_CLAMP: launch_encode_curve<TONE_CLAMP>(A, table, dither); break;
        case TONE_REINHARD: launch_encode_curve<TONE_REINHARD>(A, table, dither); break;
        case TONE_HABLE: launch_encode_curve<TONE_HABLE>(A, table, dither); break;
        case TONE_ACES: launch_encode_curve<TONE_ACES>(A, table, dither); break;
        default: break;                                // (vk_api.hip admits the four curves only)
    }
}

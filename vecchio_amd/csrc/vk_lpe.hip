// vk_lpe.hip — the kernels behind vk_lpe_* (include/vecchio_amd.h): the tag of every path of a batch kept up to date behind each bounce's
// compaction, a finished batch added to a frame of per-layer sums, and a layer's resolve.  A translation unit of its own (vk_kernels.h
// belongs to vk_api.hip): the C ABI, the handle and the argument checks stay in vk_api.hip, which calls the launchers at the end of this
// file.
//
// State, per tracker (vk_api.hip vk_lpe): a table of `capacity` tags — sig and term, 8 bytes a path id —, per pixel n_layers cells of
// four 64-bit two's-complement words — the sums of r, g, b in 2^-26 units and the count —, [pixel][layer], and one record of four
// counters kept in stripes (vk_splat.h).  Every sum is an integer add: nothing depends on the order of the lanes or on how a batch was cut.
#include <hip/hip_runtime.h>

#include "vk_emit.h"
#include "vk_lpe.h"

namespace {

constexpr int LPE_T = 256;                             // 4 waves a workgroup

}  // namespace

// lpe_record_kernel: one lane per item of a bounce, behind its compaction.  Of the 96-byte record the lane reads the last 16 bytes
// (status, lobe), of the 64-byte hit the third quarter (v, hit, front, material), and its id; it rewrites the id's tag.  An id occurs
// once per bounce, so the update is a plain load and store; ids ascend in live order, so the table access is close to coalesced.  An id
// at or beyond the table (which the host's checks exclude) is left alone.
__global__ __launch_bounds__(LPE_T) void lpe_record_kernel(LpeRecordArgs A) {
    const uint32_t j = blockIdx.x * LPE_T + threadIdx.x;
    if (j >= A.n) return;
    const uint4 tail = A.shaded[(size_t)j * 6u + 5u];          // status, lobe, _pad[2]
    const uint4 hq = A.hits[(size_t)j * 4u + 2u];              // v, hit, front, material
    const uint32_t id = A.ids[j];
    if (id >= A.capacity) return;
    const uint32_t code = lpe_event_code(tail.x, tail.y);
    uint32_t sig = 0u;
    if (A.bounce != 0u) sig = A.tags[id].x;
    A.tags[id] = make_uint2(lpe_tag_update(sig, A.bounce, code), lpe_term(hq.y, hq.w));
}

// lpe_deposit_kernel: robust_deposit_kernel (vk_robust.hip) with the layer of the result's class in place of the bucket.  One lane per
// started id of a batch with nothing live; the film's rule (vk_kernels.h deposit_lane) word for word: a candidate retired as MISS, ENDED
// or CULLED whose state's pixel lies in the frame is ours, everything else is skipped and touches nothing; one of ours with a non-finite
// acc is dropped (it counts in its cell), the others are converted as a film converts them.  The four counters are ballots: one atomic
// per wave and non-zero counter, on the wave's stripe of the record — no lane leaves before them.  The rules are read from the argument
// record with an index every lane of the wave shares.
__global__ __launch_bounds__(LPE_T) void lpe_deposit_kernel(LpeDepositArgs A) {
    const uint32_t i = blockIdx.x * LPE_T + threadIdx.x, lane = threadIdx.x & 63u;
    const bool in = i < A.n;
    uint32_t status = (uint32_t)VK_SHADE_BAD_HIT;
    uint4 s0 = make_uint4(0u, 0u, 0u, 0u), s1 = s0, s2 = s0;
    uint2 tag = make_uint2(0u, 0u);
    if (in) {
        status = A.result_status[i];
        s0 = A.result_state[(size_t)i * 3u]; s1 = A.result_state[(size_t)i * 3u + 1u]; s2 = A.result_state[(size_t)i * 3u + 2u];
        tag = A.tags[i];
    }
    const float ax = __uint_as_float(s1.x), ay = __uint_as_float(s1.y), az = __uint_as_float(s1.z);
    const bool retired = status == (uint32_t)VK_SHADE_MISS || status == (uint32_t)VK_SHADE_ENDED || status == (uint32_t)VK_PATHS_CULLED;
    const bool ours = in && retired && s2.z < A.n_pixels;
    const bool finite = isfinite(ax) && isfinite(ay) && isfinite(az);
    const float big = fmaxf(fmaxf(fabsf(ax), fabsf(ay)), fabsf(az));
    const bool large = big > ACCUM_SMALL;
    const bool dep = ours && finite;
    const unsigned long long m_dep = __ballot(dep), m_drop = __ballot(ours && !finite);
    const unsigned long long m_clamp = __ballot(dep && large && big > A.accum_clamp), m_skip = __ballot(in && !ours);
    if (lane == 0u) {
        unsigned long long *c = A.counters + (size_t)((i >> 6) & (SPLAT_STRIPES - 1u)) * SPLAT_STRIPE_WORDS;      // the wave's stripe
        if (m_dep) atomicAdd(c + 0, (unsigned long long)__popcll(m_dep));
        if (m_drop) atomicAdd(c + 1, (unsigned long long)__popcll(m_drop));
        if (m_clamp) atomicAdd(c + 2, (unsigned long long)__popcll(m_clamp));
        if (m_skip) atomicAdd(c + 3, (unsigned long long)__popcll(m_skip));
    }
    if (!ours) return;                                 // (s2.z < n_pixels and status in {0, 2, 4} from here on)
    // the first matching rule, by a loop the whole wave walks together: k is the wave's, the match is the lane's
    uint32_t layer = A.rest_layer;
    bool found = false;
    for (uint32_t k = 0; k < A.n_rules; k++) {
        const bool hit = !found && lpe_rule_matches(A.rules[k], status, s0.w, tag.x, tag.y);
        layer = hit ? A.rules[k].layer : layer;
        found = found || hit;
    }
    unsigned long long *cell = A.sums + ((size_t)s2.z * A.n_layers + (size_t)layer) * 4u;       // (layer < n_layers: create's check)
    if (dep) {
        unsigned long long fx, fy, fz;
        if (!large) {
            fx = (unsigned long long)to_fixed_small(ax); fy = (unsigned long long)to_fixed_small(ay); fz = (unsigned long long)to_fixed_small(az);
        } else {
            fx = (unsigned long long)to_fixed(ax, A.accum_clamp); fy = (unsigned long long)to_fixed(ay, A.accum_clamp);
            fz = (unsigned long long)to_fixed(az, A.accum_clamp);
        }
        atomicAdd(cell + 0, fx); atomicAdd(cell + 1, fy); atomicAdd(cell + 2, fz);
    }
    atomicAdd(cell + 3, 1ull);
}

// lpe_resolve_kernel: one lane per pixel; one layer's cell, or with LPE_ALL the layers' integer sums (wrapping, as two's complement
// does), resolved by vk_lpe.h's lpe_resolve_cell; rgb and, where asked for, the share in vk_render's f32 layout
__global__ __launch_bounds__(LPE_T) void lpe_resolve_kernel(LpeResolveArgs A) {
    const uint32_t pix = blockIdx.x * LPE_T + threadIdx.x;
    if (pix >= A.n_pixels) return;
    const long long *tab = A.sums + (size_t)pix * A.n_layers * 4u;
    unsigned long long v[4] = {0ull, 0ull, 0ull, 0ull};
    const uint32_t l0 = A.layer == LPE_ALL ? 0u : A.layer, l1 = A.layer == LPE_ALL ? A.n_layers : A.layer + 1u;
    for (uint32_t l = l0; l < l1; l++) {
        const longlong4 c = *reinterpret_cast<const longlong4 *>(tab + (size_t)l * 4u);
        v[0] += (unsigned long long)c.x; v[1] += (unsigned long long)c.y; v[2] += (unsigned long long)c.z; v[3] += (unsigned long long)c.w;
    }
    const long long w[4] = {(long long)v[0], (long long)v[1], (long long)v[2], (long long)v[3]};
    float rgb[3], share;
    lpe_resolve_cell(w, A.n, rgb, &share);
    float *o = A.rgb + (size_t)pix * 3u;
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
    if (A.share) A.share[pix] = share;
}

// ---- the launchers (vk_lpe.h): null stream, current device; sizes > 0 are the caller's to ensure
void launch_lpe_record(const LpeRecordArgs &A) {
    hipLaunchKernelGGL(lpe_record_kernel, dim3((A.n + LPE_T - 1) / LPE_T), dim3(LPE_T), 0, nullptr, A);
}

void launch_lpe_deposit(const LpeDepositArgs &A) {
    hipLaunchKernelGGL(lpe_deposit_kernel, dim3((A.n + LPE_T - 1) / LPE_T), dim3(LPE_T), 0, nullptr, A);
}

void launch_lpe_resolve(const LpeResolveArgs &A) {
    hipLaunchKernelGGL(lpe_resolve_kernel, dim3((A.n_pixels + LPE_T - 1) / LPE_T), dim3(LPE_T), 0, nullptr, A);
}

// vk_lpe.h — the kernels of vk_lpe.hip as vk_api.hip sees them: their argument records and one thin launcher each (null stream, current
// device; the caller checks hipGetLastError).  The per-lane logic — a bounce's event code, the update of a path's tag, the match of a
// result against the rules and the resolve of one cell — is host-and-device: tests/emu/emu_lpe.cpp builds it with g++.  The definition
// is include/vecchio_amd.h's ("light-path layers"); the arithmetic is f32 and built without contraction.
#ifndef VK_LPE_H
#define VK_LPE_H

#include <stdint.h>

#include "vk_math.h"        // VK_HD
#include "vk_splat.h"       // the counter record's striping (SPLAT_STRIPES, SPLAT_STRIPE_WORDS) and the reason for it

constexpr uint32_t LPE_MAX_LAYERS = 16u, LPE_MAX_RULES = 32u, LPE_COUNTERS = 4u;
constexpr uint32_t LPE_ALL = 0xFFFFFFFFu, LPE_NO_TERM = 0xFFFFFFFFu, LPE_ANY_EMITTER = 0xFFFFFFFFu;      // = VK_LPE_ALL, ...
constexpr uint64_t LPE_MAX_CELLS = 1ull << 27;         // width * height * n_layers
constexpr uint32_t LPE_SKY = 1u, LPE_FIRST_LOBE = 2u, LPE_EMIT = 5u, LPE_OTHER = 14u, LPE_BAD = 15u;       // = VK_LPE_*
// the statuses a rule may name: MISS (0), ENDED (2), CULLED (4) — the ones a deposit places
constexpr uint32_t LPE_STATUS_BITS = (1u << 0) | (1u << 2) | (1u << 4);

// One rule, as vk_lpe_rule (32 bytes): the kernels read the rules from their argument record.
struct LpeRule {
    uint32_t sig_mask, sig_value, status_mask, depth_min, depth_max, emitter, layer, _pad;
};

// A bounce's event code from the record's status and lobe as the compaction's count pass left them: MISS is the sky, BAD_HIT is bad,
// everything else (SCATTERED, ENDED, and CULLED — a roulette cull keeps its lobe) is named by the lobe that was sampled.
VK_HD uint32_t lpe_event_code(uint32_t status, uint32_t lobe) {
    if (status == 0u) return LPE_SKY;                  // VK_SHADE_MISS
    if (status == 3u) return LPE_BAD;                  // VK_SHADE_BAD_HIT
    return lobe <= 5u ? LPE_FIRST_LOBE + lobe : LPE_OTHER;
}

// The tag's first word after bounce number `bounce` of the batch (0 the first) with event `code`: nibbles 0..6 the first seven bounces,
// nibble 7 the last bounce the path took part in.  Bounce 0 forgets whatever the entry held.
VK_HD uint32_t lpe_tag_update(uint32_t sig, uint32_t bounce, uint32_t code) {
    if (bounce == 0u) return code | (code << 28);
    if (bounce < 7u) sig = (sig & ~(0xFu << (4u * bounce))) | (code << (4u * bounce));
    return (sig & 0x0FFFFFFFu) | (code << 28);
}

// The tag's second word: the material of the hit record, or LPE_NO_TERM where the record is no hit
VK_HD uint32_t lpe_term(uint32_t hit, uint32_t material) { return hit == 1u ? material : LPE_NO_TERM; }

// Does a result (status < 32, depth, tag) match the rule?
VK_HD bool lpe_rule_matches(const LpeRule &r, uint32_t status, uint32_t depth, uint32_t sig, uint32_t term) {
    return (sig & r.sig_mask) == r.sig_value && ((r.status_mask >> status) & 1u) != 0u && r.depth_min <= depth && depth <= r.depth_max &&
           (r.emitter == LPE_ANY_EMITTER || r.emitter == term);
}

// The layer of a result: the first matching rule's, `rest` without one.  status is one of the placed ones (0, 2, 4).
VK_HD uint32_t lpe_layer(const LpeRule *rules, uint32_t n_rules, uint32_t rest, uint32_t status, uint32_t depth, uint32_t sig,
                         uint32_t term) {
    for (uint32_t k = 0; k < n_rules; k++)
        if (lpe_rule_matches(rules[k], status, depth, sig, term)) return rules[k].layer;
    return rest;
}

// The resolve of one cell's four words — the sums of r, g, b in 2^-26 units and the count — for n samples a pixel
VK_HD void lpe_resolve_cell(const long long v[4], float n, float rgb[3], float *share) {
    const float inv_scale = 1.0f / 67108864.0f;        // 2^-26 (vk_emit.h ACCUM_SCALE)
    rgb[0] = ((float)v[0] * inv_scale) / n;
    rgb[1] = ((float)v[1] * inv_scale) / n;
    rgb[2] = ((float)v[2] * inv_scale) / n;
    *share = (float)v[3] / n;
}

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

// lpe_record_kernel: one lane per item of the bounce that has just been compacted
struct LpeRecordArgs {
    const uint4 *shaded;           // vk_shaded[n]: the records as the compaction's count pass left them
    const uint4 *hits;             // vk_hit[n]
    const uint32_t *ids;           // [n]: the bounce's ids in live order, each below `capacity`
    uint2 *tags;                   // [capacity]: sig, term
    uint32_t n, capacity, bounce;
};
// lpe_deposit_kernel: one lane per started id of a finished batch
struct LpeDepositArgs {
    const uint4 *result_state;     // vk_path_state[n]
    const uint32_t *result_status; // [n]
    const uint2 *tags;             // [n]
    unsigned long long *sums;      // [n_pixels][n_layers] cells of r, g, b, count
    unsigned long long *counters;  // [SPLAT_STRIPES][SPLAT_STRIPE_WORDS]: deposited, dropped, clamped, skipped in each
    uint32_t n, n_pixels, n_layers, rest_layer, n_rules;
    float accum_clamp;             // accum_clamp_for(samples_per_pixel)
    LpeRule rules[LPE_MAX_RULES];
};
// lpe_resolve_kernel: one lane per pixel
struct LpeResolveArgs {
    const long long *sums;         // [n_pixels][n_layers][4]
    float *rgb;                    // [n_pixels * 3]
    float *share;                  // [n_pixels], or null
    uint32_t n_pixels, n_layers, layer;      // layer < n_layers, or LPE_ALL
    float n;
};

void launch_lpe_record(const LpeRecordArgs &A);
void launch_lpe_deposit(const LpeDepositArgs &A);
void launch_lpe_resolve(const LpeResolveArgs &A);
#endif

#endif

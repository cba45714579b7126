// emu_lpe.cpp — TEST TOOL: the per-lane logic of vk_lpe_* on the host.  The event code, the tag update, the rule match and the resolve of
// a cell are the kernels' own — vk_lpe.h, built here with g++.  Built into tests/emu's library only.
#include "emu_query.h"
#include "../../vecchio_amd/csrc/vk_lpe.h"

static_assert(sizeof(LpeRule) == sizeof(vk_lpe_rule), "one rule, two names");

extern "C" {

// code[i] of status[i], lobe[i]
void emu_lpe_event_codes(const uint32_t *status, const uint32_t *lobe, uint64_t n, uint32_t *code) {
    for (uint64_t i = 0; i < n; i++) code[i] = lpe_event_code(status[i], lobe[i]);
}

// one bounce of lpe_record_kernel: items j < n with status, lobe, hit, material and the id ids[j] < capacity; sig and term in place
void emu_lpe_record(const uint32_t *status, const uint32_t *lobe, const uint32_t *hit, const uint32_t *material, const uint32_t *ids,
                    uint64_t n, uint64_t capacity, uint32_t bounce, uint32_t *sig, uint32_t *term) {
    for (uint64_t j = 0; j < n; j++) {
        const uint32_t id = ids[j];
        if (id >= capacity) continue;
        sig[id] = lpe_tag_update(bounce != 0u ? sig[id] : 0u, bounce, lpe_event_code(status[j], lobe[j]));
        term[id] = lpe_term(hit[j], material[j]);
    }
}

// layer[i] of the result (status[i] < 32, depth[i], sig[i], term[i]) under the rules
void emu_lpe_layers(const vk_lpe_rule *rules, uint32_t n_rules, uint32_t rest, const uint32_t *status, const uint32_t *depth,
                    const uint32_t *sig, const uint32_t *term, uint64_t n, uint32_t *layer) {
    for (uint64_t i = 0; i < n; i++)
        layer[i] = lpe_layer(reinterpret_cast<const LpeRule *>(rules), n_rules, rest, status[i], depth[i], sig[i], term[i]);
}

// cells: n * 4 values (r, g, b sums, count); rgb: n * 3 floats; share: n floats
void emu_lpe_resolve(const long long *cells, uint64_t n, uint32_t samples, float *rgb, float *share) {
    for (uint64_t p = 0; p < n; p++) lpe_resolve_cell(cells + p * 4u, (float)samples, rgb + p * 3u, share + p);
}

}  // extern "C"

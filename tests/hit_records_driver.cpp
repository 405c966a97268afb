/*
 * TEST INFRASTRUCTURE ONLY: the hit-record table of the scene image (csrc/scene_image.cpp, dscene.h DHitRec) on the
 * CPU, plain or under AddressSanitizer + UBSan (the Makefile's `hit_records_driver` / `hit_records_driver_asan`).
 * Loads a scene with the host framework, builds its image and prints one JSON object: the records, and the tables
 * they must agree with (primitives, shapes, vertex streams).  Every float is printed as its 32-bit pattern, so the
 * comparison in tests/test_hit_records.py is exact.  Touches no device.
 *   hit_records_driver <scene.xml> [key=value ...]
 */
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/amvpt_host.h"
#include "../mitsuba3-amvpt_amd/csrc/scene_image.h"

namespace amvpt {
void set_error(const std::string &msg) { std::fprintf(stderr, "error: %s\n", msg.c_str()); }
}
using namespace amvpt;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static void words(const char *name, const float *v, size_t n, const char *end = ",\n") {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < n; ++i) std::printf("%s%u", i ? ", " : "", bits(v[i]));
    std::printf("]%s", end);
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <scene.xml> [key=value ...]\n", argv[0]); return 2; }
    std::vector<std::string> keys, vals;
    for (int i = 2; i < argc; ++i) {
        const char *eq = std::strchr(argv[i], '=');
        if (!eq) return 2;
        keys.emplace_back(argv[i], eq - argv[i]);
        vals.emplace_back(eq + 1);
    }
    std::vector<const char *> kp, vp;
    for (size_t i = 0; i < keys.size(); ++i) { kp.push_back(keys[i].c_str()); vp.push_back(vals[i].c_str()); }
    amvpt_host_scene *s = amvpt_host_load_file(argv[1], kp.data(), vp.data(), (int) kp.size());
    if (!s) { std::fprintf(stderr, "load: %s\n", amvpt_host_last_error()); return 3; }
    const amvpt_scene_desc *sd = nullptr;
    const amvpt_view_desc *vd = nullptr;
    amvpt_params p;
    if (amvpt_host_describe(s, 0, 0, 0, &sd, &vd, &p) != 0) { std::fprintf(stderr, "describe failed\n"); return 3; }
    SceneImage m;
    if (validate_scene(sd) != AMVPT_OK || build_scene_image(sd, 4, 0.f, m) != AMVPT_OK) return 4;

    const uint32_t n = m.facts.n_prims;
    std::printf("{\"n_prims\": %u, \"n_hrec\": %zu, \"hrec_bytes\": %zu,\n\"prims\": [", n, m.hrec.size(), sizeof(DHitRec));
    for (uint32_t i = 0; i < n; ++i) {
        const DPrim &q = m.prims[i];
        std::printf("%s[%u, %u, %u, %u, %u]", i ? ", " : "", q.type, q.shape, bits(q.a[3]), bits(q.b[3]), bits(q.c[3]));
    }
    std::printf("],\n\"shapes\": [");
    for (uint32_t i = 0; i < m.dev.n_shapes; ++i) {
        const DShape &h = m.shapes[i];
        std::printf("%s{\"type\": %u, \"flip\": %u, \"bsdf\": %d, \"emitter\": %d, \"has_normals\": %u, \"has_uv\": %u, ",
                    i ? ", " : "", h.type, h.flip, h.bsdf, h.emitter, h.has_normals, h.has_uv);
        words("to_world", h.to_world, 12, ", "); words("to_object", h.to_object, 12, ", ");
        words("frame_n", h.frame_n, 3, ", "); words("frame_s", h.frame_s, 3, ", ");
        words("center", h.center, 3, ", "); words("radius", &h.radius, 1, "}");
    }
    std::printf("],\n");
    words("vpos", m.vpos.data(), m.vpos.size());
    words("vnrm", m.vnrm.data(), m.vnrm.size());
    words("vuv", m.vuv.data(), m.vuv.size());
    std::printf("\"hrec\": [");
    for (uint32_t i = 0; i < n; ++i) {
        const DHitRec &h = m.hrec[i];
        std::printf("%s[%u, %u, %d, %d", i ? ",\n " : "", h.kind, h.shape, h.bsdf, h.emitter);
        for (int r = 0; r < 6; ++r)
            for (int k = 0; k < 4; ++k) std::printf(", %u", bits(h.r[r][k]));
        std::printf("]");
    }
    std::printf("]}\n");
    amvpt_host_scene_free(s);
    return 0;
}

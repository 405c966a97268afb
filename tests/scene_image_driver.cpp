/*
 * TEST INFRASTRUCTURE ONLY: the scene image build (csrc/scene_image.cpp) on the CPU, plain or under
 * AddressSanitizer + UBSan (the Makefile's `scene_image_driver` / `scene_image_driver_asan`).  Loads a scene with
 * the host framework (XML -> the C-ABI descriptor the product receives), builds its image and prints one JSON
 * object: per table its element count and the 64-bit FNV-1a digest of its bytes, every scalar of the image, and a
 * few facts read out of the tables (`checks`).  Run by tests/test_scene_image.py.  Touches no device.
 *   scene_image_driver <scene.xml | empty> [leaf=N] [cost=X] [key=value ...]
 * `empty` is a descriptor without shapes, BSDFs or emitters.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/amvpt_host.h"
#include "../mitsuba3-amvpt_amd/csrc/scene_image.h"

namespace amvpt {
void set_error(const std::string &msg) { std::fprintf(stderr, "error: %s\n", msg.c_str()); }
}
using namespace amvpt;

template <class T> static void table(const char *name, const std::vector<T> &v) {
    uint64_t h = 14695981039346656037ull;
    const unsigned char *p = (const unsigned char *) v.data();
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) h = (h ^ p[i]) * 1099511628211ull;
    std::printf("  \"%s\": [%zu, \"%016llx\"],\n", name, v.size(), (unsigned long long) h);
}
static void u(const char *name, uint64_t v) { std::printf("  \"%s\": %llu,\n", name, (unsigned long long) v); }
static void f(const char *name, const float *v, int n) {
    std::printf("  \"%s\": [", name);
    for (int i = 0; i < n; ++i) std::printf(std::isfinite(v[i]) ? "%s%.9g" : "%s\"%g\"", i ? ", " : "", v[i]);
    std::printf("],\n");
}

/* facts the test asserts in words: leaf sizes, rectangles in leaves, sphere ordinals, the meshes' stream spans */
static void checks(const SceneImage &m) {
    const DScene &D = m.dev;
    uint32_t leaves[kMaxLeafPrims + 1] = {0}, rects = 0;
    for (uint32_t i = 0; i < D.n_nodes; ++i) leaves[m.nodes[i].skip_count >> kNodeCountShift]++;
    for (uint32_t i = 0; i + D.n_outer < m.facts.n_prims; ++i) rects += m.prims[i].type == PRIM_RECT;
    std::printf("  \"checks\": {\"leaf_sizes\": [");
    for (uint32_t k = 1; k <= kMaxLeafPrims; ++k) std::printf("%s%u", k > 1 ? ", " : "", leaves[k]);
    std::printf("], \"rects_in_leaves\": %u, \"sphere_ordinals\": [", rects);
    for (uint32_t i = 0; i < D.n_sph; ++i) {
        const DPrim &p = m.prims[m.sph_prims[i]];
        std::printf("%s%d", i ? ", " : "", p.type == PRIM_SPHERE ? (int) p.face : -1);
    }
    std::printf("], \"meshes\": [");
    bool first = true;
    for (size_t i = 0; i < m.shapes.size() && D.n_shapes; ++i) {
        const DShape &s = m.shapes[i];
        if (s.type != AMVPT_SHAPE_MESH) continue;
        size_t end = m.vpos.size() / 3;   /* the mesh's vertices end where the next mesh's begin */
        for (size_t j = i + 1; j < m.shapes.size(); ++j)
            if (m.shapes[j].type == AMVPT_SHAPE_MESH) { end = m.shapes[j].vbase; break; }
        bool nz = true, uz = true;
        for (size_t k = 3 * (size_t) s.vbase; k < 3 * end && k < m.vnrm.size(); ++k) nz = nz && m.vnrm[k] == 0.f;
        for (size_t k = 2 * (size_t) s.vbase; k < 2 * end && k < m.vuv.size(); ++k) uz = uz && m.vuv[k] == 0.f;
        std::printf("%s{\"vertices\": %zu, \"faces\": %u, \"has_normals\": %u, \"has_uv\": %u, \"normals_zero\": %s, "
                    "\"uv_zero\": %s}", first ? "" : ", ", end - s.vbase, s.n_faces, s.has_normals, s.has_uv,
                    nz ? "true" : "false", uz ? "true" : "false");
        first = false;
    }
    std::printf("]}\n");
}

static void print_image(const SceneImage &m) {
    const DScene &D = m.dev;
    const SceneFacts &F = m.facts;
    std::printf("{\n");
    table("nodes", m.nodes); table("prims", m.prims); table("shapes", m.shapes); table("bsdfs", m.bsdfs);
    table("emitters", m.emitters); table("vpos", m.vpos); table("vnrm", m.vnrm); table("vuv", m.vuv);
    table("faces", m.faces); table("face_area", m.face_area); table("sph_prims", m.sph_prims);
    table("boxes", m.boxes); table("box_prims", m.box_prims); table("loose_prims", m.loose_prims);
    table("outer", m.outer); table("nodes2", m.nodes2); table("nodes2h", m.nodes2h);
    u("dev.n_nodes", D.n_nodes); u("dev.n_prims", D.n_prims); u("dev.n_shapes", D.n_shapes);
    u("dev.n_emitters", D.n_emitters); f("dev.emitter_pmf", &D.emitter_pmf, 1);
    std::printf("  \"dev.environment\": %d,\n", D.environment);
    u("dev.distr", D.distr); f("dev.distr_sum", &D.distr_sum, 1); f("dev.distr_norm", &D.distr_norm, 1);
    f("dev.bs_center", D.bs_center, 3); f("dev.bs_radius", &D.bs_radius, 1);
    u("dev.lds_bytes", D.lds_bytes); u("dev.n_bsdfs", D.n_bsdfs); u("dev.tab_bytes", D.tab_bytes);
    u("dev.oct_stride", D.oct_stride); u("dev.n_sph", D.n_sph); u("dev.n_boxes", D.n_boxes);
    u("dev.n_loose", D.n_loose); u("dev.n_loose_rect", D.n_loose_rect); u("dev.n_loose_tri", D.n_loose_tri);
    u("dev.n_outer", D.n_outer); u("dev.n_nodes2", D.n_nodes2);
    f("dev.n2_center", D.n2_center, 3); f("dev.n2_scale", &D.n2_scale, 1);
    const bool null_pointers = !D.nodes && !D.prims && !D.shapes && !D.bsdfs && !D.emitters && !D.vpos && !D.vnrm &&
                               !D.vuv && !D.faces && !D.face_area && !D.sph_prims && !D.boxes && !D.box_prims &&
                               !D.loose_prims && !D.outer && !D.nodes2 && !D.nodes2h;
    u("dev.pointers_null", null_pointers);
    u("n_nodes", F.n_nodes); u("n_prims", F.n_prims); u("n_sph", F.n_sph); u("n_outer", F.n_outer);
    u("bvh_tri_only", F.bvh_tri_only); u("n_boxes", F.n_boxes); u("n_nodes2", F.n_nodes2);
    u("bvh2_depth", F.bvh2_depth); f("root_lo", F.root_lo, 3); f("root_hi", F.root_hi, 3);
    u("has_spheres", F.has_spheres); u("all_diffuse", F.all_diffuse);
    checks(m);
    std::printf("}\n");
}

int main(int argc, char **argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <scene.xml | empty> [leaf=N] [cost=X] [key=value ...]\n", argv[0]); return 2; }
    uint32_t leaf = 4;
    float cost = 0.f;
    std::vector<std::string> keys, vals;
    for (int i = 2; i < argc; ++i) {
        const char *eq = std::strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string key(argv[i], eq - argv[i]);
        if (key == "leaf") leaf = (uint32_t) std::atoi(eq + 1);
        else if (key == "cost") cost = (float) std::atof(eq + 1);
        else { keys.push_back(key); vals.emplace_back(eq + 1); }
    }
    std::vector<const char *> kp, vp;
    for (size_t i = 0; i < keys.size(); ++i) { kp.push_back(keys[i].c_str()); vp.push_back(vals[i].c_str()); }
    amvpt_host_scene *s = nullptr;
    const amvpt_scene_desc empty{};
    const amvpt_scene_desc *sd = &empty;
    if (std::strcmp(argv[1], "empty") != 0) {
        s = amvpt_host_load_file(argv[1], kp.data(), vp.data(), (int) kp.size());
        if (!s) { std::fprintf(stderr, "load: %s\n", amvpt_host_last_error()); return 3; }
        const amvpt_view_desc *vd = nullptr;
        amvpt_params p;
        if (amvpt_host_describe(s, 0, 0, 0, &sd, &vd, &p) != 0) { std::fprintf(stderr, "describe failed\n"); return 3; }
    }
    SceneImage image;
    if (validate_scene(sd) != AMVPT_OK || build_scene_image(sd, leaf, cost, image) != AMVPT_OK) return 4;
    print_image(image);
    amvpt_host_scene_free(s);
    return 0;
}

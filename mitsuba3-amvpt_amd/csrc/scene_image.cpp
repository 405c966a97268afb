/*
 * scene_image.cpp -- builds the host image of a device scene (scene_image.h), in place of the reference's Scene
 * constructor + Embree BVH build (src/render/scene.cpp:30-96, src/render/scene_embree.inl:114-116): a binned-SAH
 * binary BVH over rectangles, triangles and spheres, the primitives in BVH order and the small read-only tables.
 */
#include "scene_image.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace amvpt {

/* ---- host arithmetic for per-shape constants (same sequences as the kernels) ---- */
static inline float hdot(const float *a, const float *b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
static inline void hvec(const float *m, const float *v, float *o) { /* Transform4f * Vector3f */
    for (int i = 0; i < 3; ++i) o[i] = std::fmaf(m[i * 4 + 2], v[2], std::fmaf(m[i * 4 + 1], v[1], m[i * 4 + 0] * v[0]));
}
/* Transform::transform_affine of a point with the reference's fmadd chains (row-major 4x4) */
static inline void hpoint(const float *m, const float *p, float *o) {
    for (int i = 0; i < 3; ++i)
        o[i] = std::fmaf(m[i * 4 + 2], p[2], std::fmaf(m[i * 4 + 1], p[1], std::fmaf(m[i * 4 + 0], p[0], m[i * 4 + 3])));
}
static inline void hcross(const float *a, const float *b, float *o) {
    o[0] = std::fmaf(a[1], b[2], -(a[2] * b[1]));
    o[1] = std::fmaf(a[2], b[0], -(a[0] * b[2]));
    o[2] = std::fmaf(a[0], b[1], -(a[1] * b[0]));
}
/* x as an IEEE float16 bit pattern rounded toward -inf (up = false) or +inf (up = true); magnitudes past the
 * float16 range go to -+inf / the largest finite value on the conservative side */
static uint16_t half_dir(double x, bool up) {
    auto to_d = [](uint16_t h) -> double {
        const int e = (h >> 10) & 31, m = h & 1023;
        const double v = e == 0 ? std::ldexp((double) m, -24) : e == 31 ? INFINITY : std::ldexp((double) (1024 + m), e - 25);
        return (h & 0x8000) ? -v : v;
    };
    /* the nearest representable by bisection over the ordered bit patterns (monotone in value) */
    auto key = [](uint16_t h) -> int { return (h & 0x8000) ? -(int) (h & 0x7fff) : (int) (h & 0x7fff); };
    auto from_key = [](int k) -> uint16_t { return k < 0 ? (uint16_t) (0x8000 | (-k)) : (uint16_t) k; };
    int lo = key(0xfc00), hi = key(0x7c00);   /* -inf .. +inf */
    /* largest pattern with value <= x (down), or smallest with value >= x (up) */
    if (!up) {
        while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; if (to_d(from_key(mid)) <= x) lo = mid; else hi = mid; }
        return from_key(to_d(from_key(hi)) <= x ? hi : lo);
    }
    while (hi - lo > 1) { const int mid = lo + (hi - lo) / 2; if (to_d(from_key(mid)) >= x) hi = mid; else lo = mid; }
    return from_key(to_d(from_key(lo)) >= x ? lo : hi);
}

/* .5 * dr::norm(dr::cross(p1 - p0, p2 - p0)) (mesh.cpp:470) */
static inline float tri_area(const float *p0, const float *p1, const float *p2) {
    const float e0[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const float e1[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    float c[3];
    hcross(e0, e1, c);
    return .5f * std::sqrt(hdot(c, c));
}

/* ---- Binned SAH BVH ---- */

struct Box {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    void grow(const float *p) { for (int i = 0; i < 3; ++i) { lo[i] = std::min(lo[i], p[i]); hi[i] = std::max(hi[i], p[i]); } }
    void grow(const Box &b) { grow(b.lo); grow(b.hi); }
    float area() const {
        float d[3];
        for (int i = 0; i < 3; ++i) d[i] = std::max(hi[i] - lo[i], 0.f);
        return 2.f * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
    }
};

struct BuildPrim { Box box; float c[3]; uint32_t idx; };

/* Binary SAH tree as built (children of inner node i at left, left + 1). */
struct BNode { Box box; uint32_t left_or_first, count, axis = 0; };

#ifndef AMVPT_SAH_BINS
#define AMVPT_SAH_BINS 16   /* centroid bins per axis of the binned SAH build */
#endif

/* SAH shape: leaves of up to max_leaf primitives are kept when the split is not cheaper; a split costs
 * trav_cost primitive tests per unit of area on top of the children's tests (amvpt_set_bvh_build). */
struct Builder {
    std::vector<BuildPrim> &prims;
    const uint32_t max_leaf;
    const float trav_cost;
    std::vector<BNode> nodes;
    Builder(std::vector<BuildPrim> &p, uint32_t leaf, float cost) : prims(p), max_leaf(leaf), trav_cost(cost) {}

    static void pad(Box &b) {
        float m = 0.f;
        for (int i = 0; i < 3; ++i) m = std::max(m, std::max(std::fabs(b.lo[i]), std::fabs(b.hi[i])));
        float e = 1e-4f * (1.f + m);
        for (int i = 0; i < 3; ++i) { b.lo[i] -= e; b.hi[i] += e; }
    }
    void set(uint32_t ni, Box b) { pad(b); nodes[ni].box = b; }
    /* every split leaves both halves non-empty, so the recursion ends with leaves of <= 4 prims */
    void build(uint32_t ni, uint32_t begin, uint32_t end, int depth) {
        Box b, cb;
        for (uint32_t i = begin; i < end; ++i) { b.grow(prims[i].box); cb.grow(prims[i].c); }
        set(ni, b);
        uint32_t n = end - begin;
        if (n <= 2) { nodes[ni].left_or_first = begin; nodes[ni].count = n; return; }
        const int NB = AMVPT_SAH_BINS;
        float best_cost = INFINITY;
        int best_axis = -1, best_split = -1;
        for (int ax = 0; ax < 3; ++ax) {
            float ext = cb.hi[ax] - cb.lo[ax];
            if (!(ext > 0.f)) continue;
            Box bins[NB];
            uint32_t cnt[NB] = {0};
            for (uint32_t i = begin; i < end; ++i) {
                int k = std::min(NB - 1, (int) (NB * (prims[i].c[ax] - cb.lo[ax]) / ext));
                bins[k].grow(prims[i].box);
                cnt[k]++;
            }
            Box lb[NB], rb[NB];
            uint32_t lc[NB], rc[NB];
            Box acc;
            uint32_t ac = 0;
            for (int k = 0; k < NB; ++k) { if (cnt[k]) acc.grow(bins[k]); ac += cnt[k]; lb[k] = acc; lc[k] = ac; }
            acc = Box();
            ac = 0;
            for (int k = NB - 1; k >= 0; --k) { if (cnt[k]) acc.grow(bins[k]); ac += cnt[k]; rb[k] = acc; rc[k] = ac; }
            for (int k = 0; k < NB - 1; ++k) {
                if (!lc[k] || !rc[k + 1]) continue;
                float cost = lb[k].area() * lc[k] + rb[k + 1].area() * rc[k + 1];
                if (cost < best_cost) { best_cost = cost; best_axis = ax; best_split = k; }
            }
        }
        float leaf_cost = b.area() * n;
        best_cost += trav_cost * b.area();
        if (best_axis < 0 || (n <= max_leaf && best_cost >= leaf_cost)) {
            if (best_axis < 0) {
                /* degenerate centroids: median split on the index */
                if (n <= max_leaf) { nodes[ni].left_or_first = begin; nodes[ni].count = n; return; }
                uint32_t mid = begin + n / 2;
                uint32_t l = (uint32_t) nodes.size();
                nodes.resize(nodes.size() + 2);
                nodes[ni].left_or_first = l; nodes[ni].count = 0; nodes[ni].axis = 0;
                build(l, begin, mid, depth + 1);
                build(l + 1, mid, end, depth + 1);
                return;
            }
            nodes[ni].left_or_first = begin; nodes[ni].count = n;
            return;
        }
        float ext = cb.hi[best_axis] - cb.lo[best_axis];
        auto it = std::partition(prims.begin() + begin, prims.begin() + end, [&](const BuildPrim &p) {
            int k = std::min(NB - 1, (int) (NB * (p.c[best_axis] - cb.lo[best_axis]) / ext));
            return k <= best_split;
        });
        uint32_t mid = (uint32_t) (it - prims.begin());
        if (mid == begin || mid == end) mid = begin + n / 2;
        uint32_t l = (uint32_t) nodes.size();
        nodes.resize(nodes.size() + 2);
        nodes[ni].left_or_first = l; nodes[ni].count = 0; nodes[ni].axis = (uint32_t) best_axis;
        build(l, begin, mid, depth + 1);
        build(l + 1, mid, end, depth + 1);
    }
    /*
     * Depth-first pre-order with skip links (DNode), children in the order a ray of direction
     * octant `oct` (bit a: negative along axis a) meets them: the lower child along the split
     * axis first for a positive direction, the upper one first for a negative direction.  The
     * skip links are local to the copy, so octant copy o is the array at o * n_nodes.
     */
    void flatten(uint32_t ni, std::vector<DNode> &out, uint32_t oct = 0, uint32_t base = 0) const {
        const BNode &bn = nodes[ni];
        const uint32_t at = (uint32_t) out.size();
        DNode d{};
        for (int i = 0; i < 3; ++i) { d.lo[i] = bn.box.lo[i]; d.hi[i] = bn.box.hi[i]; }
        d.first = bn.count ? bn.left_or_first : 0u;
        out.push_back(d);
        if (!bn.count) {
            const uint32_t near = (oct >> bn.axis) & 1u;
            flatten(bn.left_or_first + near, out, oct, base);
            flatten(bn.left_or_first + (near ^ 1u), out, oct, base);
        }
        out[at].skip_count = (((uint32_t) out.size() - base) & kNodeSkipMask) | (bn.count << kNodeCountShift);
    }
    /* the two-box BVH (dscene.h DNode2) of the subtree under inner node ni, depth-first (a node, then its first
     * child's subtree, then its second's); returns ni's index in out; depth: inner nodes on the path to ni */
    uint32_t flatten2(uint32_t ni, std::vector<DNode2> &out, uint32_t depth, uint32_t &max_depth) const {
        const uint32_t at = (uint32_t) out.size();
        out.push_back(DNode2{});
        max_depth = std::max(max_depth, depth);
        uint32_t refs[2];
        for (int c = 0; c < 2; ++c) {
            const BNode &ch = nodes[nodes[ni].left_or_first + c];
            refs[c] = ch.count ? (kRef2Leaf | (ch.count << kRef2CountShift) | ch.left_or_first)
                               : flatten2(nodes[ni].left_or_first + c, out, depth + 1, max_depth);
            for (int k = 0; k < 3; ++k) {
                out[at].b[6 * c + k] = ch.box.lo[k];
                out[at].b[6 * c + 3 + k] = ch.box.hi[k];
            }
        }
        out[at].ref[0] = refs[0];
        out[at].ref[1] = refs[1];
        return at;
    }
};

static uint32_t leaf_flags(const amvpt_bsdf_desc &d) {
    if (d.type == AMVPT_BSDF_DIFFUSE) return 0x2u | 0x8000u;
    uint32_t f = 0x8u | 0x8000u;
    if (d.alpha_u != d.alpha_v) f |= 0x1000u;
    return f;
}

/* ---- Descriptor checks ---- */

static amvpt_status invalid(const char *msg) { set_error(msg); return AMVPT_ERR_INVALID; }

/* the emitter distribution, the BSDF table and the emitter table */
static amvpt_status validate_tables(const amvpt_scene_desc *d) {
    uint32_t n_env = 0;
    bool positive = false;
    for (uint32_t i = 0; i < d->emitter_count; ++i) {
        n_env += d->emitters[i].type == AMVPT_EMITTER_CONSTANT ? 1u : 0u;
        const float w = d->emitters[i].sampling_weight;
        if (!(w >= 0.f) || !std::isfinite(w)) return invalid("DiscreteDistribution: entries must be non-negative!");
        positive = positive || w > 0.f;
    }
    if (d->emitter_count && !positive) return invalid("DiscreteDistribution: no probability mass found!");
    if (n_env > 1) return invalid("Only one environment emitter can be specified per scene.");
    if (d->has_environment != n_env) return invalid("amvpt_scene_create: has_environment must count the AMVPT_EMITTER_CONSTANT emitters");
    for (uint32_t i = 0; i < d->bsdf_count; ++i) {
        const amvpt_bsdf_desc &b = d->bsdfs[i];
        if (b.type == AMVPT_BSDF_ROUGHCONDUCTOR && b.distribution != AMVPT_MICROFACET_GGX &&
            b.distribution != AMVPT_MICROFACET_BECKMANN)
            return invalid("roughconductor: unknown microfacet distribution");
        if (b.type == AMVPT_BSDF_TWOSIDED) {
            for (int k = 0; k < 2; ++k) {
                int32_t nb = b.nested[k];
                if (nb < 0 || (uint32_t) nb >= d->bsdf_count || d->bsdfs[nb].type == AMVPT_BSDF_TWOSIDED)
                    return invalid("twosided: invalid nested BSDF");
            }
        } else if (b.type > AMVPT_BSDF_TWOSIDED) {
            return invalid("unknown BSDF type");
        }
    }
    for (uint32_t i = 0; i < d->emitter_count; ++i) {
        const amvpt_emitter_desc &e = d->emitters[i];
        if (e.type == AMVPT_EMITTER_CONSTANT) {
            if (e.shape != -1) return invalid("a constant emitter is not attached to a shape (shape must be -1)");
            continue;
        }
        if (e.type != AMVPT_EMITTER_AREA) return invalid("unknown emitter type");
        if (e.shape < 0 || (uint32_t) e.shape >= d->shape_count) return invalid("emitter without a valid shape");
    }
    return AMVPT_OK;
}

static amvpt_status validate_shape(const amvpt_scene_desc *d, uint32_t i) {
    const amvpt_shape_desc &s = d->shapes[i];
    if (s.bsdf < 0 || (uint32_t) s.bsdf >= d->bsdf_count) return invalid("shape without a valid BSDF");
    if (s.emitter < -1 || (s.emitter >= 0 && (uint32_t) s.emitter >= d->emitter_count))
        return invalid("shape.emitter outside [-1, emitter_count)");
    /* the area emitter and its shape must point at each other (Shape::set_emitter) */
    if (s.emitter >= 0 && d->emitters[s.emitter].shape != (int32_t) i) return invalid("shape.emitter and emitter.shape disagree");
    if (s.type == AMVPT_SHAPE_MESH) {
        if (!s.positions || !s.faces) return invalid("mesh without positions/faces");
        for (size_t f = 0; f < 3 * (size_t) s.face_count; ++f)
            if (s.faces[f] >= s.vertex_count) return invalid("mesh face index >= vertex_count");
        if (s.emitter >= 0) {
            /* Mesh::build_pmf (mesh.cpp:448-449) / DiscreteDistribution::compute_cdf (distr_1d.h) */
            if (s.face_count == 0) return invalid("Cannot create sampling table for an empty mesh");
            float acc = 0.f;
            for (uint32_t f = 0; f < s.face_count; ++f)
                acc += tri_area(s.positions + 3 * s.faces[3 * f], s.positions + 3 * s.faces[3 * f + 1],
                                s.positions + 3 * s.faces[3 * f + 2]);
            if (!(acc > 0.f)) return invalid("DiscreteDistribution: no probability mass found!");
        }
    } else if (s.type != AMVPT_SHAPE_RECTANGLE && s.type != AMVPT_SHAPE_SPHERE) {
        return invalid("unknown shape type");
    }
    return AMVPT_OK;
}

amvpt_status validate_scene(const amvpt_scene_desc *d) {
    if ((d->shape_count && !d->shapes) || (d->bsdf_count && !d->bsdfs) || (d->emitter_count && !d->emitters))
        return invalid("amvpt_scene_create: null table with a non-zero count");
    amvpt_status st = validate_tables(d);
    for (uint32_t i = 0; st == AMVPT_OK && i < d->shape_count; ++i) st = validate_shape(d, i);
    if (st != AMVPT_OK) return st;
    for (uint32_t i = 0; i < d->emitter_count; ++i)
        if (d->emitters[i].type == AMVPT_EMITTER_AREA && d->shapes[d->emitters[i].shape].emitter != (int32_t) i)
            return invalid("shape.emitter and emitter.shape disagree");
    return AMVPT_OK;
}

/* ---- The image, step by step ---- */

/* what the steps hand on besides the image */
struct Work {
    std::vector<DPrim> scene_prims;     /* every primitive, scene order */
    std::vector<BuildPrim> bprims;      /* the BVH's primitives: its input, then in its order */
    std::vector<uint32_t> outer_idx;    /* scene_prims indices of the rectangles kept out of the BVH */
    float lo[3], hi[3];                 /* the scene's bounds (all primitives): the ray-binning grid */
};

/* p joins the scene with bounds `box` and BVH centroid c (null: the box's centre) */
static void add_prim(Work &w, DPrim p, const Box &box, const float *c) {
    BuildPrim bp;
    bp.box = box;
    bp.idx = p.pad = (uint32_t) w.scene_prims.size();
    for (int k = 0; k < 3; ++k) bp.c[k] = c ? c[k] : 0.5f * (box.lo[k] + box.hi[k]);
    w.scene_prims.push_back(p);
    w.bprims.push_back(bp);
}

/* Rectangle::update (rectangle.cpp:112-123) */
static void add_rectangle(const amvpt_shape_desc &s, uint32_t i, DShape &o, Work &w) {
    const float ex[3] = {2.f, 0.f, 0.f}, ey[3] = {0.f, 2.f, 0.f};
    hvec(s.to_world, ex, o.frame_s);
    hvec(s.to_world, ey, o.frame_t);
    /* normal through inverse_transpose = transpose(to_object) */
    float nn[3];
    for (int r = 0; r < 3; ++r)
        nn[r] = std::fmaf(s.to_object[2 * 4 + r], 1.f, std::fmaf(s.to_object[1 * 4 + r], 0.f, s.to_object[0 * 4 + r] * 0.f));
    float inv = 1.f / std::sqrt(hdot(nn, nn));
    for (int r = 0; r < 3; ++r) o.frame_n[r] = nn[r] * inv;
    float cr[3];
    hcross(o.frame_s, o.frame_t, cr);
    o.inv_area = 1.f / std::sqrt(hdot(cr, cr));
    DPrim p{};
    std::memcpy(p.a, s.to_object + 0, 16);
    std::memcpy(p.b, s.to_object + 4, 16);
    std::memcpy(p.c, s.to_object + 8, 16);
    p.type = PRIM_RECT; p.shape = i; p.face = 0;
    Box box;
    const float corners[4][3] = {{-1, -1, 0}, {-1, 1, 0}, {1, -1, 0}, {1, 1, 0}};
    for (auto &c : corners) { float v[3]; hpoint(s.to_world, c, v); box.grow(v); }
    add_prim(w, p, box, nullptr);
}

/* the mesh's streams (a mesh without normals / uvs gets a zero span once another mesh has them), its area
 * distribution and one triangle record per face */
static void add_mesh(const amvpt_shape_desc &s, uint32_t i, DShape &o, SceneImage &img, Work &w) {
    o.vbase = (uint32_t) (img.vpos.size() / 3);
    o.fbase = (uint32_t) (img.faces.size() / 3);
    o.has_normals = s.normals != nullptr;
    o.has_uv = s.texcoords != nullptr;
    img.vpos.insert(img.vpos.end(), s.positions, s.positions + 3 * (size_t) s.vertex_count);
    if (s.normals) {
        img.vnrm.resize(img.vpos.size() - 3 * (size_t) s.vertex_count, 0.f);
        img.vnrm.insert(img.vnrm.end(), s.normals, s.normals + 3 * (size_t) s.vertex_count);
    }
    if (s.texcoords) {
        img.vuv.resize(2 * (img.vpos.size() / 3 - s.vertex_count), 0.f);
        img.vuv.insert(img.vuv.end(), s.texcoords, s.texcoords + 2 * (size_t) s.vertex_count);
    }
    img.faces.insert(img.faces.end(), s.faces, s.faces + 3 * (size_t) s.face_count);
    /* Mesh::build_pmf (mesh.cpp:444-485): face areas .5 |(p1 - p0) x (p2 - p0)|, float prefix sum */
    float acc = 0.f;
    for (uint32_t f = 0; f < s.face_count; ++f) {
        const float a = tri_area(s.positions + 3 * s.faces[3 * f], s.positions + 3 * s.faces[3 * f + 1],
                                 s.positions + 3 * s.faces[3 * f + 2]);
        acc += a;
        img.face_area.push_back(a);
        img.face_area.push_back(acc);
    }
    o.n_faces = s.face_count;
    o.area_sum = acc;
    o.inv_area = acc != 0.f ? 1.f / acc : 0.f;
    for (uint32_t f = 0; f < s.face_count; ++f) {
        DPrim p{};
        const float *P0 = s.positions + 3 * s.faces[3 * f], *P1 = s.positions + 3 * s.faces[3 * f + 1],
                    *P2 = s.positions + 3 * s.faces[3 * f + 2];
        /* p0 and the two edges (the f32 differences tri_hit would form: same bits) */
        for (int k = 0; k < 3; ++k) { p.a[k] = P0[k]; p.b[k] = P1[k] - P0[k]; p.c[k] = P2[k] - P0[k]; }
        /* the spare fourth words: the face's absolute vertex indices (the hit records are built from them:
         * triangle_record) */
        for (int k = 0; k < 3; ++k) {
            const uint32_t vi = o.vbase + s.faces[3 * f + k];
            std::memcpy(k == 0 ? &p.a[3] : k == 1 ? &p.b[3] : &p.c[3], &vi, 4);
        }
        p.type = PRIM_TRI; p.shape = i; p.face = f;
        Box box;
        box.grow(P0); box.grow(P1); box.grow(P2);
        add_prim(w, p, box, nullptr);
    }
}

static void add_sphere(const amvpt_shape_desc &s, uint32_t i, DShape &o, Work &w) {
    std::memcpy(o.center, s.center, 12);
    o.radius = s.radius;
    o.inv_area = 1.f / ((4.f * 3.14159265358979323846f) * (s.radius * s.radius));
    DPrim p{};
    p.a[0] = s.center[0]; p.a[1] = s.center[1]; p.a[2] = s.center[2]; p.a[3] = s.radius;
    p.type = PRIM_SPHERE; p.shape = i; p.face = 0;
    Box box;
    for (int k = 0; k < 3; ++k) { box.lo[k] = s.center[k] - s.radius; box.hi[k] = s.center[k] + s.radius; }
    add_prim(w, p, box, s.center);
}

/* step 1: DShape records, mesh streams and area tables, and every primitive in scene order with its bounds */
static void flatten_shapes(const amvpt_scene_desc *d, SceneImage &img, Work &w) {
    img.shapes.resize(d->shape_count);
    for (uint32_t i = 0; i < d->shape_count; ++i) {
        const amvpt_shape_desc &s = d->shapes[i];
        DShape &o = img.shapes[i];
        std::memset(&o, 0, sizeof(o));
        o.type = s.type; o.flip = s.flip_normals;
        o.bsdf = s.bsdf; o.emitter = s.emitter;
        std::memcpy(o.to_world, s.to_world, 12 * sizeof(float));
        std::memcpy(o.to_object, s.to_object, 12 * sizeof(float));
        if (s.type == AMVPT_SHAPE_RECTANGLE) add_rectangle(s, i, o, w);
        else if (s.type == AMVPT_SHAPE_MESH) add_mesh(s, i, o, img, w);
        else add_sphere(s, i, o, w);   /* validate_scene admits no fourth type */
    }
    if (!img.vnrm.empty()) img.vnrm.resize(img.vpos.size(), 0.f);
    if (!img.vuv.empty()) img.vuv.resize(2 * (img.vpos.size() / 3), 0.f);
    for (int k = 0; k < 3; ++k) { w.lo[k] = INFINITY; w.hi[k] = -INFINITY; }
    for (const BuildPrim &bp : w.bprims)
        for (int k = 0; k < 3; ++k) { w.lo[k] = std::min(w.lo[k], bp.box.lo[k]); w.hi[k] = std::max(w.hi[k], bp.box.hi[k]); }
}

/* step 2: BVH scenes with a few rectangles (a room's walls and lights): the rectangles stay out of the BVH and
 * every walk tests them first (DScene::outer, dgeom.h outer_closest / outer_any) -- their boxes span the
 * scene, so every ray crossing it descended to their leaves and tested them in divergent leaf code.  In every
 * scene, the brute-force scenes' coherent walks too: config-M k_vis 44.2 -> 35.3 ms (r05u) */
static void split_outer(Work &w) {
    std::vector<BuildPrim> keep;
    for (const BuildPrim &bp : w.bprims) {
        if (w.scene_prims[bp.idx].type == PRIM_RECT) w.outer_idx.push_back(bp.idx);
        else keep.push_back(bp);
    }
    if (w.outer_idx.size() <= kOuterMax && !keep.empty()) w.bprims.swap(keep);
    else w.outer_idx.clear();
}

/* the two-box BVH of the per-lane suffix walks (at most kStack2 inner nodes deep) and its float16 form
 * (dscene.h DNode2h): the root box's centre and half extent set the frame */
static void build_two_box(const Builder &b, SceneImage &img) {
    uint32_t depth = 0;
    b.flatten2(0, img.nodes2, 1, depth);
    img.facts.bvh2_depth = depth;
    if (depth > kStack2) img.nodes2.clear();
    const Box &rb = b.nodes[0].box;
    float *center = img.dev.n2_center;
    double hmax = 0.0;
    for (int k = 0; k < 3; ++k) {
        center[k] = (float) (.5 * ((double) rb.lo[k] + (double) rb.hi[k]));
        hmax = std::max(hmax, .5 * ((double) rb.hi[k] - (double) rb.lo[k]));
    }
    const float scale = img.dev.n2_scale = hmax > 0.0 ? (float) (1.0 / hmax) : 1.f;
    for (const DNode2 &n : img.nodes2) {
        DNode2h q{};
        uint16_t hv[12];
        for (int c = 0; c < 2; ++c)
            for (int k = 0; k < 3; ++k) {
                const double lo = ((double) n.b[6 * c + k] - (double) center[k]) * (double) scale;
                const double hi = ((double) n.b[6 * c + 3 + k] - (double) center[k]) * (double) scale;
                hv[6 * c + k] = half_dir(lo, false);
                hv[6 * c + 3 + k] = half_dir(hi, true);
            }
        for (int w = 0; w < 6; ++w) q.h[w] = (uint32_t) hv[2 * w] | ((uint32_t) hv[2 * w + 1] << 16);
        q.ref[0] = n.ref[0];
        q.ref[1] = n.ref[1];
        img.nodes2h.push_back(q);
    }
}

/* step 3: the threaded BVH over w.bprims (SAH build, flatten), for BVHs read per lane from device memory the
 * eight octant copies and the two-box tree, and prims[] in BVH order */
static amvpt_status build_bvh(Work &w, uint32_t max_leaf, float trav_cost, SceneImage &img) {
    if (w.bprims.empty()) {
        /* one inner node with an empty box: every ray misses it and skips to the end */
        DNode root{};
        root.lo[0] = root.lo[1] = root.lo[2] = 1.f;
        root.hi[0] = root.hi[1] = root.hi[2] = -1.f;
        root.first = 0;
        root.skip_count = 1u;
        img.nodes.push_back(root);
        return AMVPT_OK;
    }
    Builder b(w.bprims, max_leaf, trav_cost);
    b.nodes.resize(1);
    b.build(0, 0, (uint32_t) w.bprims.size(), 0);
    img.nodes.reserve(b.nodes.size());
    b.flatten(0, img.nodes);
    if (img.nodes.size() > kNodeSkipMask) { set_error("BVH too large (more than 2^28 nodes)"); return AMVPT_ERR_INVALID; }
    const uint32_t n0 = (uint32_t) img.nodes.size();
    /* the bytes the LDS-staged tier copies (DScene::lds_bytes: the outer rectangles follow the BVH's primitives
     * in prims[]), so a BVH is staged or gets the copies and the two-box tree, never neither */
    const uint64_t lds_b = (uint64_t) n0 * sizeof(DNode) + (w.bprims.size() + w.outer_idx.size()) * sizeof(DPrim);
    const bool per_lane = n0 > kUniformNodeLimit && lds_b > kLdsSceneBytes;
    /* per-lane walks of BVHs that are neither wave-uniform nor LDS-staged read the copy of their ray's
     * direction octant: nearest child first, so the closest hit shrinks the box-test range early */
    if (per_lane && (uint64_t) n0 * 8 <= kNodeSkipMask) {
        img.nodes.reserve((size_t) n0 * 8);
        for (uint32_t o = 1; o < 8; ++o) b.flatten(0, img.nodes, o, o * n0);
        img.dev.oct_stride = n0;
    }
    /* (leaves addressable in a reference; more than kUniformNodeLimit nodes: the root is an inner node) */
    if (per_lane && w.bprims.size() <= kRef2FirstMask) build_two_box(b, img);
    img.prims.resize(w.bprims.size());
    for (size_t i = 0; i < w.bprims.size(); ++i) img.prims[i] = w.scene_prims[w.bprims[i].idx];
    return AMVPT_OK;
}

/* step 4: the outer rectangles follow the BVH's primitives in prims[]; outer[] holds copies with that index */
static void append_outer(const Work &w, SceneImage &img) {
    for (uint32_t idx : w.outer_idx) {
        DPrim q = w.scene_prims[idx];
        q.type |= (uint32_t) img.prims.size() << 8;
        img.outer.push_back(q);
        img.prims.push_back(w.scene_prims[idx]);
    }
    img.dev.n_outer = img.facts.n_outer = (uint32_t) img.outer.size();
    img.facts.n_prims = (uint32_t) img.prims.size();
    if (img.prims.empty()) img.prims.resize(1); /* keep a valid pointer */
}

/* step 5: the BSDF table */
static void build_bsdfs(const amvpt_scene_desc *d, SceneImage &img) {
    img.bsdfs.resize(d->bsdf_count);
    for (uint32_t i = 0; i < d->bsdf_count; ++i) {
        const amvpt_bsdf_desc &s = d->bsdfs[i];
        DBsdf &o = img.bsdfs[i];
        std::memset(&o, 0, sizeof(o));
        o.type = s.type; o.distribution = s.distribution;
        o.sample_visible = s.sample_visible; o.has_spec = s.has_specular_reflectance;
        o.nested0 = s.nested[0]; o.nested1 = s.nested[1];
        std::memcpy(o.refl, s.reflectance, 12);
        o.alpha_u = s.alpha_u; o.alpha_v = s.alpha_v;
        std::memcpy(o.eta, s.eta, 12);
        std::memcpy(o.k, s.k, 12);
        std::memcpy(o.spec, s.specular_reflectance, 12);
        if (s.type == AMVPT_BSDF_TWOSIDED) {
            uint32_t f0 = leaf_flags(d->bsdfs[s.nested[0]]), f1 = leaf_flags(d->bsdfs[s.nested[1]]);
            o.flags = ((f0 & ~0x10000u) | 0x8000u) | ((f1 & ~0x8000u) | 0x10000u);
        } else {
            o.flags = leaf_flags(s);
        }
    }
}

/* ConstantBackgroundEmitter::set_scene (constant.cpp:73-88): the bounding sphere of Scene::bbox()
 * (union of Shape::bbox(): rectangle corners, mesh vertices, sphere center -+ radius), center =
 * (min + max) / 2, radius = |center - max| enlarged by (1 + RayEpsilon), at least RayEpsilon */
static void scene_bsphere(const amvpt_scene_desc *d, float center[3], float &radius) {
    const float ray_eps = 1500.f * 5.9604644775390625e-8f;   /* math.h:18-23: 1500 * 2^-24 */
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool any = false;
    auto expand = [&](const float p[3]) {
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], p[k]); hi[k] = std::max(hi[k], p[k]); }
        any = true;
    };
    for (uint32_t i = 0; i < d->shape_count; ++i) {
        const amvpt_shape_desc &s = d->shapes[i];
        if (s.type == AMVPT_SHAPE_RECTANGLE) {
            const float corners[4][3] = {{-1.f, -1.f, 0.f}, {1.f, -1.f, 0.f}, {1.f, 1.f, 0.f}, {-1.f, 1.f, 0.f}};
            for (auto &c : corners) { float w[3]; hpoint(s.to_world, c, w); expand(w); }
        } else if (s.type == AMVPT_SHAPE_MESH) {
            for (uint32_t v = 0; v < s.vertex_count; ++v) expand(s.positions + 3 * (size_t) v);
        } else {
            const float a[3] = {s.center[0] - s.radius, s.center[1] - s.radius, s.center[2] - s.radius};
            const float b[3] = {s.center[0] + s.radius, s.center[1] + s.radius, s.center[2] + s.radius};
            expand(a); expand(b);
        }
    }
    if (!any) { center[0] = center[1] = center[2] = 0.f; radius = ray_eps; return; }
    for (int k = 0; k < 3; ++k) center[k] = (hi[k] + lo[k]) * .5f;
    const float dx = center[0] - hi[0], dy = center[1] - hi[1], dz = center[2] - hi[2];
    radius = std::sqrt(std::fmaf(dz, dz, std::fmaf(dy, dy, dx * dx)));
    radius = std::max(ray_eps, radius * (1.f + ray_eps));
}

/* step 6: the emitter table with its sampling distribution, and the environment's bounding sphere */
static void build_emitters(const amvpt_scene_desc *d, SceneImage &img) {
    DScene &D = img.dev;
    img.emitters.resize(std::max<uint32_t>(1, d->emitter_count));
    bool distr = false;
    float cdf_acc = 0.f;
    D.environment = -1;
    for (uint32_t i = 0; i < d->emitter_count; ++i) {
        DEmitter &e = img.emitters[i];
        std::memset(&e, 0, sizeof(e));
        e.shape = d->emitters[i].shape;
        e.type = d->emitters[i].type;
        std::memcpy(e.radiance, d->emitters[i].radiance, 12);
        e.weight = d->emitters[i].sampling_weight;
        cdf_acc += e.weight;   /* DiscreteDistribution::compute_cdf: dr::prefix_sum in float */
        e.cdf = cdf_acc;
        distr = distr || e.weight != 1.f;
        if (e.type == AMVPT_EMITTER_CONSTANT) D.environment = (int32_t) i;
    }
    D.n_emitters = d->emitter_count;
    D.emitter_pmf = d->emitter_count ? 1.f / (float) d->emitter_count : 0.f;
    D.distr = distr ? 1u : 0u;
    D.distr_sum = d->emitter_count ? img.emitters[d->emitter_count - 1].cdf : 0.f;
    D.distr_norm = D.distr_sum != 0.f ? 1.f / D.distr_sum : 0.f;
    if (D.environment >= 0) scene_bsphere(d, D.bs_center, D.bs_radius);
}

/* step 7: sphere ordinals (DScene::sph_prims): the record's `face` field, unused by spheres otherwise */
static void number_spheres(SceneImage &img) {
    for (uint32_t i = 0; i < (uint32_t) img.prims.size(); ++i)
        if (img.prims[i].type == PRIM_SPHERE) {
            img.prims[i].face = (uint32_t) img.sph_prims.size();
            img.sph_prims.push_back(i);
        }
    img.dev.n_sph = img.facts.n_sph = (uint32_t) img.sph_prims.size();
}

/* ---- hit records (dscene.h DHitRec): the hit-independent part of compute_si (dgeom.h), operation for operation
 * as the kernels formed it per hit -- fmaf where dmath.h has fmadd / fmsub, 1.0f / sqrt for rsqrt_, 1.0f / x for
 * rcp, the same operand order (this unit is built with -ffp-contract=off) ---- */
static inline uint32_t hbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float hfloat(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline float hmulsign(float a, float b) { return hfloat(hbits(a) ^ (hbits(b) & 0x80000000u)); }
static inline float hmulsign_neg(float a, float b) { return hfloat(hbits(a) ^ (~hbits(b) & 0x80000000u)); }
/* the s of coord_sys (dmath.h; vector.h:116-136) */
static void hcoord_s(const float *n, float *s) {
    const float sg = hmulsign(1.f, n[2]), a = -(1.0f / (sg + n[2])), b = n[0] * n[1] * a;
    s[0] = hmulsign((n[0] * n[0]) * a, n[2]) + 1.f;
    s[1] = hmulsign(b, n[2]);
    s[2] = hmulsign_neg(n[0], n[2]);
}

static void triangle_record(const SceneImage &img, const DPrim &p, const DShape &s, DHitRec &h) {
    const uint32_t vi[3] = {hbits(p.a[3]), hbits(p.b[3]), hbits(p.c[3])};   /* absolute vertex indices (add_mesh) */
    const float *P[3] = {&img.vpos[3 * (size_t) vi[0]], &img.vpos[3 * (size_t) vi[1]], &img.vpos[3 * (size_t) vi[2]]};
    float e1[3], e2[3], c[3], n[3], dp_du[3];
    for (int k = 0; k < 3; ++k) { e1[k] = P[1][k] - P[0][k]; e2[k] = P[2][k] - P[0][k]; }
    hcross(e1, e2, c);
    const float il = 1.0f / std::sqrt(hdot(c, c));
    for (int k = 0; k < 3; ++k) n[k] = c[k] * il;
    hcoord_s(n, dp_du);
    if (s.has_uv) {
        const float *u0 = &img.vuv[2 * (size_t) vi[0]], *u1 = &img.vuv[2 * (size_t) vi[1]], *u2 = &img.vuv[2 * (size_t) vi[2]];
        const float d0x = u1[0] - u0[0], d0y = u1[1] - u0[1], d1x = u2[0] - u0[0], d1y = u2[1] - u0[1];
        const float det = std::fmaf(d0x, d1y, -(d0y * d1x));
        if (det != 0.f) {
            const float inv_det = 1.0f / det;
            for (int k = 0; k < 3; ++k) dp_du[k] = std::fmaf(d1y, e1[k], -(d0y * e2[k])) * inv_det;
        }
    }
    if (s.has_normals) h.kind |= kHitNormals;
    for (int v = 0; v < 3; ++v) {
        for (int k = 0; k < 3; ++k) {
            h.r[v][k] = P[v][k];
            h.r[3 + v][k] = s.has_normals ? img.vnrm[3 * (size_t) vi[v] + k] : 0.f;
        }
        h.r[v][3] = s.flip ? -n[v] : n[v];
        h.r[3 + v][3] = dp_du[v];
    }
}

/* step 9: one hit record per primitive, in prims[] order */
static void build_hit_records(SceneImage &img) {
    img.hrec.resize(img.prims.size());
    for (uint32_t i = 0; i < img.facts.n_prims; ++i) {
        const DPrim &p = img.prims[i];
        const DShape &s = img.shapes[p.shape];
        DHitRec &h = img.hrec[i];
        std::memset(&h, 0, sizeof(h));
        h.kind = p.type | (s.flip ? kHitFlip : 0u);
        h.shape = p.shape; h.bsdf = s.bsdf; h.emitter = s.emitter;
        if (p.type == PRIM_RECT) {
            for (int k = 0; k < 3; ++k) { h.r[0][k] = s.to_world[4 * k + 3]; h.r[1][k] = s.frame_n[k]; h.r[2][k] = s.frame_s[k]; }
        } else if (p.type == PRIM_TRI) {
            triangle_record(img, p, s, h);
        } else {
            std::memcpy(h.r[0], s.center, 12);
            h.r[0][3] = s.radius;
            std::memcpy(h.r[1], s.to_object, 16);
            std::memcpy(h.r[2], s.to_object + 4, 16);
            for (int k = 0; k < 3; ++k) std::memcpy(h.r[3 + k], s.to_world + 4 * k, 12);
        }
    }
}

static constexpr uint32_t kBrutePrimsHost = 48;  /* dgeom.h kBrutePrims: brute-force scenes have no BVH walk */
/*
 * Box meshes (dscene.h DBox): a mesh shape of 12 triangles whose vertices map, through the shape's
 * to_object (in double), to corners of [-1, 1]^3 within 1e-5, every triangle lying in one face plane, two
 * triangles per face covering its four corners -- the `cube` plugin's mesh (cube.cpp:105-160) under any
 * affine to_world.  Boxes whose box-space coordinates would magnify the walks' rounding are left to the plain
 * scan: the screen maps a ray's ORIGIN into box space, and the suffix rays start anywhere on the scene's
 * surfaces, so the bound is the box's conditioning (largest row norm of to_object) times (1 + the largest
 * coordinate magnitude of the whole scene, desc_extent), not of the box's own vertices: a small
 * cube on a ground plane 1000 units wide would have its box-space origins at ~1e4 and f32 rounding near kBoxEps.
 * prims[] is in BVH order; box_prims / loose_prims hold copies with the BVH index in `type`'s upper bits.
 */
/* the largest coordinate magnitude of any primitive of the scene (world space): mesh vertices, rectangle corners
 * (to_world of (+-1, +-1, 0)), sphere centres +- radius */
static double desc_extent(const amvpt_scene_desc *d) {
    double e = 0.0;
    for (uint32_t i = 0; i < d->shape_count; ++i) {
        const amvpt_shape_desc &s = d->shapes[i];
        if (s.type == AMVPT_SHAPE_MESH && s.positions) {
            for (size_t k = 0; k < (size_t) 3 * s.vertex_count; ++k) e = std::max(e, (double) std::fabs(s.positions[k]));
        } else if (s.type == AMVPT_SHAPE_RECTANGLE) {
            for (int c = 0; c < 4; ++c) {
                const double x = (c & 1) ? 1.0 : -1.0, y = (c & 2) ? 1.0 : -1.0;
                for (int r = 0; r < 3; ++r)
                    e = std::max(e, std::fabs(s.to_world[4 * r] * x + s.to_world[4 * r + 1] * y + s.to_world[4 * r + 3]));
            }
        } else if (s.type == AMVPT_SHAPE_SPHERE) {
            for (int r = 0; r < 3; ++r) e = std::max(e, (double) std::fabs(s.center[r]) + (double) std::fabs(s.radius));
        }
    }
    return e;
}
static void find_boxes(const amvpt_scene_desc *d, const std::vector<DPrim> &prims, std::vector<DBox> &boxes,
                       std::vector<DPrim> &box_prims, std::vector<DPrim> &loose) {
    const double extent = desc_extent(d);
    std::vector<int> in_box(prims.size(), 0);
    for (uint32_t i = 0; i < d->shape_count; ++i) {
        const amvpt_shape_desc &s = d->shapes[i];
        if (s.type != AMVPT_SHAPE_MESH || s.face_count != 12 || !s.positions || !s.faces) continue;
        std::vector<uint32_t> tris;
        for (uint32_t pi = 0; pi < (uint32_t) prims.size(); ++pi)
            if (prims[pi].type == PRIM_TRI && prims[pi].shape == i) tris.push_back(pi);
        if (tris.size() != 12) continue;
        double M[12], cond = 0.0, wmax = 0.0;
        for (int k = 0; k < 12; ++k) M[k] = (double) s.to_object[k];
        for (int r = 0; r < 3; ++r)
            cond = std::max(cond, std::sqrt(M[4 * r] * M[4 * r] + M[4 * r + 1] * M[4 * r + 1] + M[4 * r + 2] * M[4 * r + 2]));
        bool ok = true;
        int n_on[6] = {0, 0, 0, 0, 0, 0};
        uint32_t ftri[12];
        uint32_t corners[6] = {0, 0, 0, 0, 0, 0};   /* per face: the (b, c) corners its triangles touch, 4 bits */
        for (uint32_t pi : tris) {
            const uint32_t f = prims[pi].face;
            double b[3][3];
            for (int v = 0; v < 3; ++v) {
                const float *w = s.positions + 3 * (size_t) s.faces[3 * f + v];
                for (int r = 0; r < 3; ++r) {
                    b[v][r] = M[4 * r] * w[0] + M[4 * r + 1] * w[1] + M[4 * r + 2] * w[2] + M[4 * r + 3];
                    wmax = std::max(wmax, (double) std::fabs(w[r]));
                    if (std::fabs(std::fabs(b[v][r]) - 1.0) > 1e-5) ok = false;
                }
            }
            int axis = -1;
            for (int a = 0; a < 3; ++a)
                if ((b[0][a] > 0) == (b[1][a] > 0) && (b[0][a] > 0) == (b[2][a] > 0)) { axis = a; break; }
            if (!ok || axis < 0) { ok = false; break; }
            const int face = 2 * axis + (b[0][axis] > 0 ? 1 : 0);
            if (n_on[face] >= 2) { ok = false; break; }
            ftri[2 * face + n_on[face]++] = pi;
            const int bx = (axis + 1) % 3, cx = (axis + 2) % 3;
            for (int v = 0; v < 3; ++v) corners[face] |= 1u << ((b[v][bx] > 0 ? 1 : 0) + (b[v][cx] > 0 ? 2 : 0));
        }
        for (int f = 0; ok && f < 6; ++f) ok = n_on[f] == 2 && corners[f] == 15u;
        if (!ok || cond * (1.0 + std::max(wmax, extent)) >= 100.0) continue;
        DBox B{};
        for (int k = 0; k < 12; ++k) B.m[k] = (float) M[k];
        for (int k = 0; k < 12; ++k) {
            DPrim q = prims[ftri[k]];
            q.type = PRIM_TRI | (ftri[k] << 8);
            box_prims.push_back(q);
            in_box[ftri[k]] = 1;
        }
        boxes.push_back(B);
    }
    /* (with no box, every primitive is loose: the typed scans and the rectangle cull still apply) */
    /* grouped by type (rectangles, triangles, spheres), BVH order within a group: the walks loop over each
     * group with its own test (the closest-hit rule does not depend on the order) */
    for (uint32_t type : {(uint32_t) PRIM_RECT, (uint32_t) PRIM_TRI, (uint32_t) PRIM_SPHERE})
        for (uint32_t pi = 0; pi < (uint32_t) prims.size(); ++pi)
            if (!in_box[pi] && prims[pi].type == type) {
                DPrim q = prims[pi];
                q.type |= pi << 8;
                loose.push_back(q);
            }
}

/* step 8: box meshes and loose primitives of brute-force scenes (dgeom.h box_walk) */
static void build_boxes(const amvpt_scene_desc *d, SceneImage &img) {
    DScene &D = img.dev;
    if (img.prims.size() <= kBrutePrimsHost) find_boxes(d, img.prims, img.boxes, img.box_prims, img.loose_prims);
    D.n_boxes = img.facts.n_boxes = (uint32_t) img.boxes.size();
    D.n_loose = (uint32_t) img.loose_prims.size();
    for (const DPrim &q : img.loose_prims) {
        D.n_loose_rect += (q.type & 0xffu) == PRIM_RECT ? 1u : 0u;
        D.n_loose_tri += (q.type & 0xffu) == PRIM_TRI ? 1u : 0u;
    }
}

/* step 10: the remaining scalars, then one zero element in every empty table (keep a valid pointer) */
static void finish(const amvpt_scene_desc *d, const Work &w, SceneImage &img) {
    DScene &D = img.dev;
    SceneFacts &F = img.facts;
    F.has_spheres = D.n_sph > 0;
    F.bvh_tri_only = !w.bprims.empty();
    for (const BuildPrim &bp : w.bprims) F.bvh_tri_only = F.bvh_tri_only && w.scene_prims[bp.idx].type == PRIM_TRI;
    F.all_diffuse = d->bsdf_count > 0;
    for (uint32_t i = 0; i < d->bsdf_count; ++i) F.all_diffuse = F.all_diffuse && d->bsdfs[i].type == AMVPT_BSDF_DIFFUSE;
    std::memcpy(F.root_lo, w.bprims.empty() ? img.nodes[0].lo : w.lo, sizeof(F.root_lo));
    std::memcpy(F.root_hi, w.bprims.empty() ? img.nodes[0].hi : w.hi, sizeof(F.root_hi));
    D.n_nodes = F.n_nodes = D.oct_stride ? D.oct_stride : (uint32_t) img.nodes.size();
    D.n_nodes2 = F.n_nodes2 = (uint32_t) img.nodes2.size();
    D.n_prims = (uint32_t) img.prims.size();
    D.n_shapes = d->shape_count;
    D.n_bsdfs = d->bsdf_count;
    const uint32_t tb = tab_round(d->shape_count * (uint32_t) sizeof(DShape)) +
                        tab_round(d->bsdf_count * (uint32_t) sizeof(DBsdf)) +
                        tab_round(d->emitter_count * (uint32_t) sizeof(DEmitter));
    D.tab_bytes = tb <= kTabBytes ? tb : 0u;
    D.lds_bytes = (uint32_t) ((size_t) D.n_nodes * sizeof(DNode) + img.prims.size() * sizeof(DPrim));
    auto keep = [](auto &v, size_t n) { if (v.empty()) v.resize(n); };   /* n zero elements */
    keep(img.vpos, 3); keep(img.vnrm, 3); keep(img.vuv, 2); keep(img.faces, 3); keep(img.face_area, 2);
    keep(img.outer, 1); keep(img.sph_prims, 1); keep(img.boxes, 1); keep(img.box_prims, 1); keep(img.loose_prims, 1);
    keep(img.nodes2, 1); keep(img.nodes2h, 1); keep(img.hrec, 1);
}

/* the steps keep this order: each reads what the ones before it left */
amvpt_status build_scene_image(const amvpt_scene_desc *d, uint32_t max_leaf, float trav_cost, SceneImage &img) {
    img = SceneImage();
    img.dev.n2_scale = 1.f;
    Work w;
    flatten_shapes(d, img, w);
    split_outer(w);
    const amvpt_status st = build_bvh(w, max_leaf, trav_cost, img);
    if (st != AMVPT_OK) return st;
    append_outer(w, img);
    build_bsdfs(d, img);
    build_emitters(d, img);
    number_spheres(img);
    build_boxes(d, img);
    build_hit_records(img);
    finish(d, w, img);
    return AMVPT_OK;
}

uint32_t count_boxes(const amvpt_scene_desc *d) {
    SceneImage img;
    Work w;
    flatten_shapes(d, img, w);   /* find_boxes reads type, shape and face: scene order serves */
    find_boxes(d, w.scene_prims, img.boxes, img.box_prims, img.loose_prims);
    return (uint32_t) img.boxes.size();
}

} // namespace amvpt

/*
 * scene_image.h -- the host image of a device scene: every table amvpt_scene_create uploads and every scalar of
 * DScene, built from the descriptor by host arithmetic alone (scene_image.cpp: plain C++, no device, so it runs on
 * any host and under sanitizers: tests/scene_image_driver.cpp).
 */
#pragma once
#include "internal.h"

namespace amvpt {

struct SceneImage {
    /* one vector per DScene pointer, as uploaded: an empty table holds one zero element (a valid pointer) */
    std::vector<DNode> nodes;
    std::vector<DPrim> prims, box_prims, loose_prims, outer;
    std::vector<DShape> shapes;
    std::vector<DBsdf> bsdfs;
    std::vector<DEmitter> emitters;
    std::vector<float> vpos, vnrm, vuv, face_area;
    std::vector<uint32_t> faces, sph_prims;
    std::vector<DBox> boxes;
    std::vector<DNode2> nodes2;
    std::vector<DNode2h> nodes2h;
    std::vector<DHitRec> hrec;   /* one per entry of prims[] */
    DScene dev{};      /* every scalar set, every pointer null */
    SceneFacts facts;
};

/* Descriptor checks (no device needed): every index the image build or the kernels follow is in range. */
amvpt_status validate_scene(const amvpt_scene_desc *d);
/* The image of a validated descriptor; max_leaf / trav_cost: the SAH shape (amvpt_set_bvh_build). */
amvpt_status build_scene_image(const amvpt_scene_desc *d, uint32_t max_leaf, float trav_cost, SceneImage &img);
/* Box meshes of a validated descriptor (dscene.h DBox), whatever its primitive count. */
uint32_t count_boxes(const amvpt_scene_desc *d);

} // namespace amvpt

// rtw_common.cpp -- error reporting shared by every C entry point of librtw.so.
#include "rtw_common.h"

namespace rtw {

namespace {
thread_local std::string g_last_error;
}

void set_error(const std::string& msg) { g_last_error = msg; }

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

const char* last_error() { return g_last_error.c_str(); }

}  // namespace rtw

// 64-bit FNV-1a over the world's contents (rtw.h): plain fields and table bytes, never pointers.
extern "C" RTW_API int rtw_world_fingerprint(const rtw_world* w, uint64_t* out) {
    if (!w || !out) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "null argument");
    uint64_t h = 0xCBF29CE484222325ull;
    auto bytes = [&](const void* p, size_t n) {
        const uint8_t* b = static_cast<const uint8_t*>(p);
        for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001B3ull;
    };
    bool bad = false;
    auto table = [&](int32_t count, const void* p, size_t each) {
        bytes(&count, sizeof(count));
        if (count > 0 && !p) bad = true;
        else if (count > 0) bytes(p, (size_t)count * each);
    };
    bytes(&w->camera, sizeof(w->camera));
    bytes(&w->background, sizeof(w->background));
    bytes(&w->has_light, sizeof(w->has_light));
    bytes(&w->light, sizeof(w->light));
    bytes(&w->root, sizeof(w->root));
    table(w->node_count, w->nodes, sizeof(rtw_bvh_node));
    table(w->leaf_count, w->leaves, sizeof(rtw_leaf));
    table(w->sphere_count, w->spheres, sizeof(rtw_sphere));
    table(w->rect_count, w->rects, sizeof(rtw_rect));
    table(w->box_count, w->boxes, sizeof(rtw_box));
    table(w->triangle_count, w->triangles, sizeof(rtw_triangle));
    table(w->material_count, w->materials, sizeof(rtw_material));
    table(w->texture_count, w->textures, sizeof(rtw_texture));
    bytes(&w->image_count, sizeof(w->image_count));
    if (w->image_count > 0 && !w->images) bad = true;
    for (int32_t i = 0; !bad && i < w->image_count; ++i) {
        const rtw_image& im = w->images[i];
        bytes(&im.width, sizeof(im.width));
        bytes(&im.height, sizeof(im.height));
        if (im.width > 0 && im.height > 0) {
            if (!im.rgb) bad = true;
            else bytes(im.rgb, (size_t)im.width * (size_t)im.height * 3);
        }
    }
    table(w->perlin_count, w->perlins, sizeof(rtw_perlin));
    if (bad) return rtw::fail(RTW_ERR_INVALID_ARGUMENT, "invalid world: a table with a count but no data");
    *out = h;
    return RTW_OK;
}

extern "C" RTW_API const char* rtw_last_error(void) { return rtw::last_error(); }
extern "C" RTW_API int rtw_version(void) { return RTW_ABI_VERSION; }

/*
 * rtw.h -- C ABI of the MI355X path tracer (librtw.so).
 *
 * Drop-in boundary: the reference's hot path is the Rust library function
 *
 *     pub fn render(image_size: Size2i, thread_count: usize, samples_per_pixel: usize,
 *                   max_depth: i32, world: &World, render_mode: RenderMode) -> Vec<Color>
 *                                                              (src/lib/rendering.rs:121-128)
 *
 * `rtw_render` replaces it.  `World` (rendering.rs:12-17) crosses the boundary as the flat,
 * pointer-and-count struct `rtw_world` below: the camera (camera.rs:154-164), the one top-level
 * BVH the builder produces (world_builder.rs:282 -> hittable.rs:352-357) over its flattened leaf
 * list (world_builder.rs:291-328), the primitive / material / texture tables, the background
 * (background_color.rs:3-6) and the optional light-sampling rect
 * (world_scattering_distribution.rs:4-9).  A Rust caller serialises its World into this struct
 * inside the lib crate (several fields are private there); INTEGRATION.md shows that shim.
 *
 * Everything is plain C: pointers, sizes, int status codes.  No torch types.  All entry points
 * return RTW_OK (0) or an RTW_ERR_* code; `rtw_last_error()` returns a thread-local message.
 * The reference panics instead of returning errors; the Rust shim maps non-zero to panic!.
 *
 * Host-side scene construction (WorldBuilder / Camera builder / OBJ loader / demo worlds:
 * src/app/worlds/world_builder.rs, demo_worlds.rs, src/app/obj_loader.rs, camera.rs:11-152) is
 * exported too, so C++ and Python hosts can build the same worlds the Rust app builds; see the
 * second half of the file.
 */
#ifndef RTW_H
#define RTW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTW_API __attribute__((visibility("default")))
#define RTW_ABI_VERSION 2

/* ---- status codes ------------------------------------------------------------------------ */
#define RTW_OK 0
#define RTW_ERR_INVALID_ARGUMENT 1
#define RTW_ERR_NO_DEVICE 2
#define RTW_ERR_HIP 3
#define RTW_ERR_OUT_OF_MEMORY 4
#define RTW_ERR_UNSUPPORTED 5
#define RTW_ERR_IO 6
#define RTW_ERR_PARSE 7

/* ---- enums (values are ABI) ------------------------------------------------------------- */
/* Geometry (hittable.rs:104-110) */
#define RTW_GEOM_SPHERE 0
#define RTW_GEOM_RECT 1
#define RTW_GEOM_BOX 2
#define RTW_GEOM_TRIANGLE 3
/* RectPlane (rect_geometry.rs:8-21): (p0, p1, n) axes = Xy (0,1,2), Xz (0,2,1), Yz (1,2,0) */
#define RTW_PLANE_XY 0
#define RTW_PLANE_XZ 1
#define RTW_PLANE_YZ 2
/* Material (material.rs:42-49) */
#define RTW_MAT_LAMBERT 0
#define RTW_MAT_METAL 1
#define RTW_MAT_DIELECTRIC 2
#define RTW_MAT_DIFFUSE_LIGHT 3
#define RTW_MAT_ISOTROPIC 4
/* Texture (texture.rs:3-20) */
#define RTW_TEX_SOLID 0
#define RTW_TEX_CHECKER 1
#define RTW_TEX_MARBLE 2
#define RTW_TEX_IMAGE 3
/* BackgroundColor (background_color.rs:3-6) */
#define RTW_BG_SKY 0
#define RTW_BG_SOLID 1
/* RenderMode (rendering.rs:94-98) */
#define RTW_MODE_DEFAULT 0
#define RTW_MODE_NORMALS 1
/* Leaf wrappers produced by finish_internal (world_builder.rs:305-316) */
#define RTW_LEAF_VOLUME 1u    /* SceneElement::VolumeGeometry (density < 1) */
#define RTW_LEAF_TRANSFORM 2u /* wrapped in SceneElement::Transformation */
#define RTW_LEAF_ANIMATION 4u /* wrapped (outermost) in SceneElement::Animation */
/* Output layouts of rtw_render_device */
#define RTW_LAYOUT_IMAGE 0 /* W*H*3 f32, row-major from the top-left pixel */
#define RTW_LAYOUT_TILES 1 /* this partition's tiles only, tile-major, tile_w*tile_h*3 f32 each */

/* ---- flat World ------------------------------------------------------------------------- */
/* BVH node (hittable.rs:345-351).  Children: >= 0 node index, < 0 leaf ~index (= -1 - leaf). */
typedef struct rtw_bvh_node {
    float min[3];
    float max[3];
    int32_t axis;
    int32_t left;
    int32_t right;
} rtw_bvh_node;

/* One flattened scene leaf (world_builder.rs:305-316):
 *   Animation(velocity)? ( Transformation(offset, y_sin, y_cos)? ( Volume | Surface ) ) */
typedef struct rtw_leaf {
    int32_t geom_kind;  /* RTW_GEOM_* */
    int32_t geom_index; /* index into the per-kind table */
    int32_t material;   /* material index (phase function for volumes) */
    uint32_t flags;     /* RTW_LEAF_* */
    float neg_inv_density; /* VolumeGeometry::neg_inv_density = -1/density (hittable.rs:305) */
    float offset[3];       /* Transformation (transformations.rs:4-8) */
    float y_sin;
    float y_cos;
    float velocity[3]; /* Animation (hittable.rs:117) */
} rtw_leaf;

typedef struct rtw_sphere { /* sphere_geometry.rs:6-9 */
    float center[3];
    float radius;
} rtw_sphere;
typedef struct rtw_rect { /* rect_geometry.rs:25-30 */
    int32_t plane;
    float dist;
    float r0[2];
    float r1[2];
} rtw_rect;
typedef struct rtw_box { /* aabb.rs:10-13 used as a primitive */
    float min[3];
    float max[3];
} rtw_box;
typedef struct rtw_triangle { /* triangle_geometry.rs:6-10 */
    float positions[3][3];
    float normals[3][3];
    float uvs[3][2];
} rtw_triangle;

typedef struct rtw_material {
    int32_t kind;    /* RTW_MAT_* */
    int32_t texture; /* albedo / emit texture, -1 for dielectric */
    float fuzz;      /* metal */
    float index_of_refraction; /* dielectric */
} rtw_material;

typedef struct rtw_texture {
    int32_t kind; /* RTW_TEX_* */
    float color[3];      /* solid */
    float inv_frequency; /* checker */
    int32_t even, odd;   /* checker: texture indices */
    float scale;         /* marble */
    int32_t perlin;      /* marble: perlin index */
    int32_t image;       /* image: image index */
} rtw_texture;

typedef struct rtw_image { /* image::RgbImage, row 0 = top */
    int32_t width, height;
    const uint8_t* rgb; /* width*height*3 */
} rtw_image;

#define RTW_PERLIN_MAX_POINTS 256
typedef struct rtw_perlin { /* perlin.rs:10-16, bits <= 8 */
    int32_t bits;
    float ranvec[RTW_PERLIN_MAX_POINTS][3];
    uint32_t perm_x[RTW_PERLIN_MAX_POINTS];
    uint32_t perm_y[RTW_PERLIN_MAX_POINTS];
    uint32_t perm_z[RTW_PERLIN_MAX_POINTS];
} rtw_perlin;

typedef struct rtw_camera { /* camera.rs:154-164 (all fields, private ones included) */
    float position[3];
    float upper_left_corner[3];
    float unit_right[3];
    float unit_up[3];
    float scaled_right[3];
    float scaled_up[3];
    float lens_radius;
    float time0, time1;
    float shutter_pace[2];
} rtw_camera;

typedef struct rtw_background {
    int32_t kind; /* RTW_BG_* */
    float color[3];
} rtw_background;

typedef struct rtw_world {
    rtw_camera camera;
    rtw_background background;
    int32_t has_light; /* scattering_distribution_provider.is_some() */
    rtw_rect light;    /* WorldScatteringDistributionProvider::Rect */
    int32_t root;      /* BVH initial_index: node index, or ~leaf for a one-leaf scene */
    int32_t node_count;
    const rtw_bvh_node* nodes;
    int32_t leaf_count;
    const rtw_leaf* leaves;
    int32_t sphere_count;
    const rtw_sphere* spheres;
    int32_t rect_count;
    const rtw_rect* rects;
    int32_t box_count;
    const rtw_box* boxes;
    int32_t triangle_count;
    const rtw_triangle* triangles;
    int32_t material_count;
    const rtw_material* materials;
    int32_t texture_count;
    const rtw_texture* textures;
    int32_t image_count;
    const rtw_image* images;
    int32_t perlin_count;
    const rtw_perlin* perlins;
} rtw_world;

/* The deepest BVH the device walks: nodes on the longest root-to-leaf path (its per-lane stack). */
#define RTW_MAX_BVH_DEPTH 32
/* The longest texture chain the device follows: checkers in a row plus the texture that ends them. */
#define RTW_MAX_TEXTURE_CHAIN 64

/* The validator every upload runs first (host only: it needs no device and touches none).  It reads
 * `world` and nothing else, follows no index before it has checked it, and answers
 *   RTW_OK                    *depth (when not NULL) = nodes on the longest root-to-leaf path, 0 for a
 *                             one-leaf world; every read the device and the oracle make of the tables
 *                             is then in bounds;
 *   RTW_ERR_INVALID_ARGUMENT  the world is not one the reference can express (list below);
 *   RTW_ERR_UNSUPPORTED       a well-formed tree deeper than RTW_MAX_BVH_DEPTH.
 * On an error rtw_last_error() reads "invalid world: <table>[<index>].<field> <what>" (no index for the
 * world's own fields: "invalid world: root ...", "invalid world: light.plane ...") and *depth is left alone.
 * A world is accepted when
 *   - every count is >= 0, leaf_count >= 1, and every table with a count > 0 has its pointer;
 *   - root is a node index < node_count, or ~leaf of a leaf < leaf_count;
 *   - the nodes reachable from root form a binary tree: axis 0..2, children in range, every node and every
 *     leaf referenced exactly once (the reference's builder makes no other tree: none shared, none left
 *     out, no cycle), so node_count == leaf_count - 1;
 *   - leaves: geom_kind 0..3, geom_index inside that kind's table, material < material_count, no flag
 *     above RTW_LEAF_ANIMATION;
 *   - materials: kind 0..4 and, except for a dielectric (whose texture is ignored, -1 by convention),
 *     texture < texture_count;
 *   - textures: kind 0..3; a checker's even and odd, an image texture's image and a marble's perlin inside
 *     their tables (the fields a kind does not use are ignored); checkers form no cycle and no chain of
 *     more than RTW_MAX_TEXTURE_CHAIN textures, the one that ends it included;
 *   - perlins: bits 1..8 and perm_x / perm_y / perm_z [0 .. 2^bits) all < 2^bits (the rest is never read);
 *   - images: width, height >= 1 and rgb not NULL;
 *   - rects[].plane, and light.plane when has_light (0 or 1), are RTW_PLANE_*; a light's r0 and r1 are
 *     increasing ranges within +-2^30 (the reference samples them with gen_range, which panics otherwise);
 *   - camera.time0 <= camera.time1, both finite and their difference too (gen_range again, unless equal);
 *   - node bounds, sphere centres and radii, rect distances, leaf offsets, leaf velocity x the largest
 *     ray time, and the camera position are no NaN and at most 2^30 in magnitude. */
RTW_API int rtw_world_check(const rtw_world* world, int32_t* depth);

/* ---- render parameters ------------------------------------------------------------------- */
typedef struct rtw_render_params {
    int32_t width, height;      /* image_size: Size2i (width, height >= 2) */
    uint32_t samples_per_pixel; /* >= 1 */
    int32_t max_depth;          /* ray_color depth budget (rendering.rs:19-20) */
    int32_t render_mode;        /* RTW_MODE_* */
    int32_t layout;             /* RTW_LAYOUT_* (rtw_render_device only) */
    uint64_t seed;              /* replaces StdRng::from_entropy (rendering.rs:160) */
    int32_t tile_width;         /* 0 -> 8 */
    int32_t tile_height;        /* 0 -> 8 */
    int32_t part_index;         /* this caller renders tiles t with t % part_count == part_index */
    int32_t part_count;         /* 0 -> 1 */
    /* thread_count of rendering::render (rendering.rs:121-128): the reference splits the samples
     * into thread_count planes (split_work_tasks, rendering.rs:222-237: the first spp % T planes
     * take one sample more, planes of 0 samples are dropped), averages each plane over its own
     * sample count and merges them last-plane-first (merge_planes, rendering.rs:239-252).  The
     * device reproduces that arithmetic exactly (plane t sums samples start_t.. in order).
     * 0 -> 1 (one plane: sum / spp). */
    int32_t thread_count;
    int32_t reserved0; /* must be 0 */
} rtw_render_params;

/* Traversal statistics of one render (for the algorithmic-bytes model). */
typedef struct rtw_render_stats {
    uint64_t samples;
    uint64_t rays;
    uint64_t node_visits;
    uint64_t sphere_tests, rect_tests, box_tests, triangle_tests;
    uint64_t sphere_hits, rect_hits, box_hits, triangle_hits; /* closest hits */
    uint64_t material_reads;
    uint64_t texel_reads;
} rtw_render_stats;

typedef struct rtw_gpu_world rtw_gpu_world; /* a World resident in one device's HBM */

/* ---- render API (librtw.so) -------------------------------------------------------------- */
RTW_API int rtw_version(void);
RTW_API const char* rtw_last_error(void);
RTW_API int rtw_device_count(int* count);

/* Drop-in for rendering::render: uploads `world` to `device`, renders every pixel, copies the
 * linear radiance (W*H*3 f32, row-major from the top-left pixel) into host `out_rgb`. */
RTW_API int rtw_render(const rtw_world* world, const rtw_render_params* params, int device,
                       float* out_rgb);

/* rtw_render with progress reports, the analogue of the reference's progress thread
 * (rendering.rs:140-157): cb(done_samples, total_samples, user) is called from the calling
 * thread about every 50 ms while the frame renders (done_samples counts finished work items of
 * RTW_CHUNK samples), and once more with done == total before returning.  cb == NULL behaves
 * like rtw_render. */
typedef void (*rtw_progress_fn)(uint64_t done_samples, uint64_t total_samples, void* user);
RTW_API int rtw_render_progress(const rtw_world* world, const rtw_render_params* params, int device,
                                float* out_rgb, rtw_progress_fn cb, void* user);

/* rtw_render on several GPUs of one node (one call may use several devices).  The
 * frame's interleaved tile_width x tile_height tiles (params->tile_*, default 8x8) are split over the
 * list: entry i renders the tiles t with t % n_devices == i on devices[i], on its own host thread; the
 * tile buffers reach devices[0] by peer copy over xGMI and are placed there (rtw_untile_device); the
 * image is copied into host `out_rgb` as rtw_render does.  A device may repeat (several partitions on
 * one GPU).  Bit-identical to rtw_render for every list (per-(pixel, sample) RNG streams).
 * params->part_index / part_count must be 0 / 0 or 1: the call partitions the frame itself. */
RTW_API int rtw_render_devices(const rtw_world* world, const rtw_render_params* params, const int* devices,
                               int n_devices, float* out_rgb);
/* The same, resident: rtw_multi_create uploads the world to every listed device once;
 * rtw_multi_render renders one frame and leaves the W*H*3 f32 image in d_image on devices[0]
 * (synchronous: it returns when the image is complete). */
typedef struct rtw_multi rtw_multi;
RTW_API int rtw_multi_create(const rtw_world* world, const int* devices, int n_devices, rtw_multi** out);
RTW_API int rtw_multi_render(rtw_multi* m, const rtw_render_params* params, float* d_image);
RTW_API int rtw_multi_release(rtw_multi* m);
/* Tile-buffer copies this rtw_multi made with hipMemcpyPeerAsync (partitions on a device other than
 * devices[0]; with RTW_MULTI_FORCE_PEER=1 in the environment at rtw_multi_create, every partition's:
 * a same-device peer copy, so one GPU runs the path distinct devices take).  Diagnostics only. */
RTW_API int rtw_multi_peer_copies(const rtw_multi* m, uint64_t* copies);

/* Resident path: upload once, render many times into device memory. */
RTW_API int rtw_world_upload(const rtw_world* world, int device, rtw_gpu_world** out);
RTW_API int rtw_world_release(rtw_gpu_world* gw);
/* The dynamic ray-fetch threshold this world's renders settled on (tuned on the device during
 * the first long render; 0 while still exploring).  Synchronous; performance only -- images do
 * not depend on it. */
RTW_API int rtw_world_tuning(rtw_gpu_world* gw, int* trace_min);
/* The render-kernel variant this world's last render launched: LDS mode (0 scene in HBM, 1 tree +
 * leaf records in LDS, 2 + triangle records), leaf kinds (0 plain spheres .. 4 any), texture
 * kinds (0 solid only, 1 any) and search tree (0 the reference BVH, 1 the kernel's SAH tree with
 * the reference-order proof and fallback); -1 each before the first render.
 * Diagnostics only. */
RTW_API int rtw_world_kernel(rtw_gpu_world* gw, int* lds_mode, int* leaf_kinds, int* tex_kinds, int* tree);
/* Where that launch put its tables: out[0] shading tables (leaf_info, materials) in LDS, out[1] texture
 * table in LDS, out[2] the SAH walk's proof boxes in LDS, out[3] the generic leaf tables (transforms,
 * spheres, boxes) in LDS, out[4] the shared drain's mailbox present (each 1 or 0; 0: read from HBM / L2, or
 * no mailbox), out[5] the triangle prefix (leading mesh leaves whose records the kernel makes up), out[6]
 * the launch's dynamic LDS bytes, out[7] 1 when it walked the SAH tree; -1 each before the first render.
 * Diagnostics only. */
RTW_API int rtw_world_last_launch_lds(rtw_gpu_world* gw, int32_t out[8]);
/* The exact template name of that kernel, as profilers print it inside the demangled symbol
 * ("render_kernel<false, 1, 0, 0, false, false>": counting variant, LDS mode, leaf kinds, texture kinds,
 * generic leaf tables in LDS, whole-pixel work items), NUL-terminated into buf[0..cap); "" before the
 * first render.  The leaf-list kernel's single-sample variants (WP false) carry a seventh place, their camera
 * batch; its whole-pixel variants keep six:
 * "render_kernel_pl<false, 1, 0, 0, false, false, true>"; RTW_CAMERA_BATCH=0 selects the "false" kernel.
 * The solid-texture batch kernel that also shades the camera hit in the fill carries an eighth place, put
 * before the batch's: "render_kernel_pl<false, 1, 0, 0, false, false, true, true>"; RTW_FIRST_BOUNCE=0
 * selects the seven-place batch kernel.
 * RTW_ERR_INVALID_ARGUMENT if cap is too small.  Diagnostics only (bench.py matches PMC rows by it). */
RTW_API int rtw_world_kernel_name(rtw_gpu_world* gw, char* buf, int cap);
/* Tests: the camera batch's counters on `device`, summed over the render launches since the last reset:
 * out3 = fills, samples stored, samples picked.  "Stored" is a valid sample prepared by a fill; "picked" is a
 * sample that left the fill's custody: a record handed to a lane, or a sample the fill finished itself (first
 * bounce).  The last two are equal, and equal to the samples rendered, when every work item was traced exactly
 * once; kernels without the batch add nothing.  Synchronous; reset != 0 zeroes them. */
RTW_API int rtw_debug_park_counts(int device, unsigned long long* out3, int reset);
/* Tests: what the fills of the first-bounce kernel did with their samples, summed like the counters above:
 * out3 = samples finished in the fill (no record), bounce records parked, unsolved records parked.  Their sum
 * is "stored"; kernels without the first bounce add nothing.  Synchronous; reset != 0 zeroes them. */
RTW_API int rtw_debug_fill_counts(int device, unsigned long long* out3, int reset);
/* The shape of this world's last frame (rtw_render_device / rtw_render on it): render-kernel launches,
 * whether the work items were whole pixels (1: samples summed in registers, no colour buffer, DESIGN.md
 * 5.5b; 0: single samples through the colour buffer), and the dynamic-fetch threshold it ran with (the
 * world's tuned one once chosen, else the default: 32, 16 for whole-pixel frames, or RTW_TRACE_MIN);
 * -1 each before the first frame.  Synchronous; diagnostics only. */
RTW_API int rtw_world_last_frame(rtw_gpu_world* gw, int* launches, int* whole_pixel, int* trace_min);
/* The primary rays' per-tile leaf lists (include/rtw_beam.h) of that frame: tiles
 * with a non-empty list, tiles with an empty list (their camera rays miss), tiles left to the SAH walk
 * (list above the cap, degenerate beam), and the mean list length over the tiles that have one.  All 0
 * when the frame used no lists (world out of scope, RTW_PRIMARY_LISTS=0, a kernel variant without them;
 * then the kernel's name is "render_kernel<...>", with lists "render_kernel_pl<...>", same arguments). */
RTW_API int rtw_world_last_frame_lists(rtw_gpu_world* gw, int* listed, int* empty, int* walked, double* mean_len);
/* The lists the world holds, those of its last frame's shape: tile count (0: none), the cap and the builder
 * kernel's time in ms; count[n_tiles] (entries, or -1: the tile takes the walk) and list[n_tiles * cap] are
 * filled when not NULL.  Synchronous; tests and diagnostics. */
RTW_API int rtw_world_primary_lists(rtw_gpu_world* gw, int32_t* n_tiles, int32_t* cap, double* build_ms,
                                    int32_t* count, int32_t* list);
/* The same lists built on the host by the same arithmetic (needs no GPU): params' width, height and tile
 * shape; count[tiles], list[tiles * cap].  RTW_ERR_UNSUPPORTED unless every leaf is a plain cullable sphere. */
RTW_API int rtw_primary_lists_host(const rtw_world* world, const rtw_render_params* params, int32_t cap,
                                   int32_t* count, int32_t* list);
/* Renders this partition's tiles into device buffer `d_out` (layout per params->layout) on
 * `stream` (a hipStream_t, NULL = default stream).  Asynchronous: returns after the launch. */
RTW_API int rtw_render_device(rtw_gpu_world* gw, const rtw_render_params* params, float* d_out,
                              void* stream);
/* ---- progressive accumulation ------------------------------------------------------------- */
/* An accumulator keeps one partition's per-slot running sums of sample colours on the device, so a
 * frame can grow: add samples in batches, resolve (sum / samples) at any point, export the state
 * and import it later into an accumulator of the same world, geometry, depth, mode and seed.  A
 * sample's RNG stream is keyed by (seed, pixel, sample) and the sums are added in sample order, so
 * after adds of n1, n2, ... samples the resolved image is bit-identical to a one-shot render at
 * samples_per_pixel = n1 + n2 + ... (and to the reference at that spp).
 *
 * The accumulator is tied to one resident world and to params' geometry (width, height, tiles,
 * part), max_depth, render_mode, seed and layout; params->samples_per_pixel is ignored and may be 0.
 * params->thread_count > 1 is RTW_ERR_UNSUPPORTED: the reference's plane split depends on the final
 * spp (split_work_tasks, rendering.rs:222-237), so a prefix of such a frame is not a frame; 0 and 1
 * are accepted.  The accumulator owns its sums (and squares); the world's own scratch stays the
 * one-shot frames', so one-shot frames and several accumulators of one world may interleave freely
 * (they run one at a time, in issue order).  rtw_world_release takes the device state of the world's
 * live accumulators with it: such an accumulator then refuses every call but rtw_accum_get_info and
 * rtw_accum_release (a host whose collector frees the two in either order stays safe).
 *
 * Work items: where a one-shot frame would take whole-pixel items (rtw_world_last_frame), an
 * accumulator without moments takes them too (the lane continues the slot's running sum), except
 * on worlds whose kernel keeps the generic leaf tables in LDS (wrapped, box or volume leaves: the
 * "true" in the fifth place of rtw_world_kernel_name), which add single samples.  One with
 * RTW_ACCUM_MOMENTS always takes single-sample items, its squares being summed in the accumulate
 * pass; so does one with RTW_ACCUM_FINITE, whose filter sees the samples one by one in that pass (a
 * whole-pixel launch sums inside the render kernel and cannot filter).  rtw_world_last_frame reports an
 * add like a frame.  DESIGN.md 5.5c.
 *
 * Adaptive sampling (RTW_ACCUM_ADAPTIVE, needs RTW_ACCUM_MOMENTS).  The accumulator also
 * keeps one uint32_t tile_stop per local tile (the partition's tiles in slot order): 0 = the tile is
 * active, any other value = the sample count at which it stopped.  A stopped tile stays stopped, so every
 * active tile holds exactly info.samples samples and a tile's count is
 *   tile_stop[t] ? tile_stop[t] : info.samples.
 * rtw_accum_adapt stops converged tiles, rtw_accum_add renders the active tiles only, and the resolves
 * divide by the tile's own count.  The contract moves from the frame to the tile: a tile that stopped at
 * n holds, bit for bit, the pixels of a frame at samples_per_pixel = n (and of the reference at that
 * spp); the stop decision is a fixed f32 expression of the sums and squares (include/rtw_adapt.h), so a
 * host can replay the whole run; the stop map is part of the output.  Like every accumulator with
 * moments, an adaptive one takes single-sample work items.
 *
 * Finite-sample accumulation (RTW_ACCUM_FINITE; include/rtw_finite.h has the definition).  The
 * reference's 0/0 pdf quirk makes an occasional whole sample NaN, and one NaN sample turns its pixel's sum NaN for
 * good.  With this flag the accumulate pass leaves out every sample with a channel that is NaN or +-inf: it adds
 * nothing to the sums (and squares) and is not counted.  The accumulator also keeps one uint32_t `kept` per slot,
 * the samples that entered the sums; rejected = the slot's sample count - kept.  The resolves, the noise estimate
 * and rtw_accum_adapt divide by the pixel's own kept in place of the sample count (kept == 0 resolves to +0.0;
 * kept < 2 has no finite standard error and is left out of the noise mean and of a tile's E, as every pixel with
 * a non-finite value is).  The counts are part of the output, as the stop map is.  The flag combines with
 * RTW_ACCUM_MOMENTS and RTW_ACCUM_ADAPTIVE and works without either; it changes nothing for accumulators created
 * without it, nor for rtw_render*.  A finite accumulator always takes single-sample work items, as one with
 * moments does: the accumulate pass is where samples are seen one by one, so a whole-pixel launch cannot filter.
 * On a pixel with no rejected sample every output is the plain accumulator's, bit for bit.  Dropping samples
 * biases the estimate (the dropped paths carried energy): the exact reference image stays the plain accumulator's.
 *
 * Sample clamping (RTW_ACCUM_CLAMP, needs RTW_ACCUM_FINITE; include/rtw_clamp.h has the definition, DESIGN.md
 * 5.5j).  The accumulator has a level L (f32, 0 < L < inf; rtw_accum_create_clamp).  The accumulate pass scales
 * every finite sample whose largest channel exceeds L so that it equals L (the hue is kept, no accumulated channel
 * exceeds L), and keeps, per slot, `clamped` (one uint32_t: the samples it scaled) and `lost` (three f32: the sum of
 * what it took out of them).  Sums, squares and kept hold the clamped samples, so every resolve, the noise estimate
 * and rtw_accum_adapt are the finite accumulator's on them; rtw_accum_resolve_clamp_loss gives lost / kept, the
 * mean radiance the clamp removed from each pixel.  The flag combines with RTW_ACCUM_MOMENTS and
 * RTW_ACCUM_ADAPTIVE.  Such an accumulator always takes single-sample work items, as a finite one does.  On a
 * pixel with no clamped sample every value is the finite accumulator's, bit for bit.  Clamping biases the estimate
 * (it removes energy): nothing changes for accumulators created without the flag, nor for rtw_render*. */
typedef struct rtw_accum rtw_accum;
#define RTW_ACCUM_MOMENTS 1u  /* also keep per-channel sums of squares (the noise estimate) */
#define RTW_ACCUM_ADAPTIVE 2u /* per-tile stop map: converged tiles take no more samples */
#define RTW_ACCUM_FINITE 4u   /* leave non-finite samples out of the sums; per-slot kept counts */
#define RTW_ACCUM_CLAMP 8u    /* scale finite samples above the level down to it; per-slot clamped counts and lost */
typedef struct rtw_accum_info { /* all fields fixed-width, no padding; also the checkpoint header */
    uint32_t version; /* 1 */
    uint32_t flags;   /* RTW_ACCUM_* */
    int32_t width, height, tile_width, tile_height, part_index, part_count;
    int32_t max_depth, render_mode;
    uint32_t samples;  /* samples added so far, per pixel */
    uint32_t reserved; /* 0; with RTW_ACCUM_CLAMP the bits of the f32 level (an import of another level is refused) */
    uint64_t seed;
    uint64_t world_fingerprint; /* rtw_world_fingerprint of the uploaded world */
    int64_t slots;              /* floats per state array = 3 * slots */
} rtw_accum_info;

/* 64-bit FNV-1a over the world's contents in declaration order: camera, background, has_light,
 * light, root; every count followed by its table's bytes; per image its width, height and pixels.
 * Pointers are not hashed.  Host only.  rtw_world_upload stores it in the rtw_gpu_world. */
RTW_API int rtw_world_fingerprint(const rtw_world* w, uint64_t* out);
RTW_API int rtw_accum_create(rtw_gpu_world* gw, const rtw_render_params* params, uint32_t flags,
                             rtw_accum** out);
/* An accumulator with RTW_ACCUM_CLAMP (flags must hold it and RTW_ACCUM_FINITE, else RTW_ERR_INVALID_ARGUMENT naming
 * the flags) of clamp level `level`; a level that is NaN, <= 0 or infinite is refused with a message naming clamp.
 * rtw_accum_create refuses the flag: it has no level.  Otherwise as rtw_accum_create. */
RTW_API int rtw_accum_create_clamp(rtw_gpu_world* gw, const rtw_render_params* params, uint32_t flags, float level,
                                   rtw_accum** out);
RTW_API int rtw_accum_release(rtw_accum* a);
/* Renders samples [samples, samples + n) of every slot and adds their colours to the running sums
 * in sample order (with RTW_ACCUM_MOMENTS also sq = sq + c * c per channel, product and sum each
 * rounded to f32).  Asynchronous on `stream`; one add may be several launches (colour-buffer
 * budget, RTW_CHUNK).  n == 0 does nothing; samples + n beyond 32 bits is
 * RTW_ERR_INVALID_ARGUMENT.  An adaptive accumulator renders samples [samples, samples + n) of its
 * active tiles only (the sums, squares and colours of stopped tiles are not touched) and advances
 * info.samples only when at least one tile is active; with no active tile the call does nothing and
 * returns RTW_OK.  While every tile is active it runs exactly the launches of a plain moments
 * accumulator; with fewer, the launch walks the active tiles in the world's learned cost order
 * (costliest first; tile order before one is learned), each tile's samples together. */
RTW_API int rtw_accum_add(rtw_accum* a, uint32_t n_samples, void* stream);
RTW_API int rtw_accum_get_info(rtw_accum* a, rtw_accum_info* out); /* host bookkeeping, no sync */
/* sum / (float)samples into device buffer d_out, in params->layout.  Non-destructive; needs
 * samples >= 1.  Asynchronous.
 * (Adaptive: here and in the standard error and the noise estimate, `samples` is the tile's own count.) */
RTW_API int rtw_accum_resolve(rtw_accum* a, float* d_out, void* stream);
/* The standard error of the mean per channel (needs RTW_ACCUM_MOMENTS and samples >= 2), in f32:
 * nf = (float)samples; mean = sum / nf; d = sq - sum * mean; var = (d < 0 ? 0 : d) / (float)(samples - 1);
 * se = sqrt(var / nf).  Same layout as the resolve.  Asynchronous. */
RTW_API int rtw_accum_resolve_stderr(rtw_accum* a, float* d_out, void* stream);
/* One scalar for the partition: the f64 mean over its pixels of the f32 value
 * e = ((se_r + se_g) + se_b) / (((mean_r + mean_g) + mean_b) + 0.01f), leaving out pixels whose e is
 * not finite; *pixels_counted = pixels that entered the mean (0: *noise = 0).  Same conditions as the
 * stderr.  Synchronous. */
RTW_API int rtw_accum_noise(rtw_accum* a, void* stream, double* noise, int64_t* pixels_counted);
/* The samples each pixel holds (the tile's count), one uint32_t per pixel (RTW_LAYOUT_IMAGE; pixels of other
 * partitions are left alone) or per slot (RTW_LAYOUT_TILES; padding slots get 0).  Any accumulator: without
 * RTW_ACCUM_ADAPTIVE every count is info.samples.  Asynchronous. */
RTW_API int rtw_accum_resolve_samples(rtw_accum* a, uint32_t* d_out, void* stream);
/* RTW_ACCUM_ADAPTIVE only (else RTW_ERR_INVALID_ARGUMENT), samples >= 2 and min_samples >= 2.  For every active
 * tile: E = the maximum over the tile's owned pixels of the f32 value e of rtw_accum_noise, leaving out pixels
 * whose e is not finite (no finite pixel: E = 0); if samples >= min_samples and E <= target then
 * tile_stop[t] = samples.  Returns the tiles and the owned pixels that are still active.  The arithmetic is
 * include/rtw_adapt.h's; rtw_adapt_tiles_host runs it on host arrays.  Synchronous. */
RTW_API int rtw_accum_adapt(rtw_accum* a, float target, uint32_t min_samples, void* stream, int64_t* active_tiles,
                            int64_t* active_pixels);
/* The same decision on exported state, without a GPU: sums and squares as rtw_accum_export gives them for
 * params' geometry (width, height, tile shape, part), tile_stop[local tiles] updated in place. */
RTW_API int rtw_adapt_tiles_host(const float* sums, const float* squares, const rtw_render_params* params,
                                 uint32_t samples, float target, uint32_t min_samples, uint32_t* tile_stop);
/* Copies the stop map (one entry per local tile = slots / (tile_width * tile_height)) to the host.
 * RTW_ACCUM_ADAPTIVE only.  Synchronous. */
RTW_API int rtw_accum_tile_stops(rtw_accum* a, uint32_t* host_stop);
/* Copies the sums (and, with moments, the squares; host_squares may be NULL otherwise) to the host,
 * 3 * slots floats each, in slot order (tile-major); padding slots of edge tiles hold zeros.
 * Synchronous. */
RTW_API int rtw_accum_export(rtw_accum* a, float* host_sums, float* host_squares);
/* Sets the sums (and squares) and the sample count from an exported state.  `info` must match the
 * accumulator's own version, flags, geometry, max_depth, render_mode, seed, world fingerprint and
 * slots, else RTW_ERR_INVALID_ARGUMENT with a message naming the field.  Synchronous. */
RTW_API int rtw_accum_import(rtw_accum* a, const rtw_accum_info* info, const float* host_sums,
                             const float* host_squares);
/* The checkpoint of an adaptive accumulator: rtw_accum_export plus the stop map, and its import.  `info` is
 * checked as in rtw_accum_import (its flags hold RTW_ACCUM_ADAPTIVE; rtw_accum_info stays version 1); a
 * tile_stop entry of 1 or above info->samples is refused with a message naming tile_stop.  Plain
 * rtw_accum_import on an adaptive accumulator is refused too (it has no tile_stop to set). */
RTW_API int rtw_accum_export_adaptive(rtw_accum* a, float* host_sums, float* host_squares, uint32_t* host_tile_stop);
RTW_API int rtw_accum_import_adaptive(rtw_accum* a, const rtw_accum_info* info, const float* host_sums,
                                      const float* host_squares, const uint32_t* host_tile_stop);
/* RTW_ACCUM_FINITE only (else RTW_ERR_INVALID_ARGUMENT): the kept count of each pixel or slot, laid out and padded
 * as rtw_accum_resolve_samples lays out the sample counts.  Asynchronous. */
RTW_API int rtw_accum_resolve_kept(rtw_accum* a, uint32_t* d_out, void* stream);
/* One export / import pair for every flag combination: sums always; squares with RTW_ACCUM_MOMENTS, tile_stop
 * with RTW_ACCUM_ADAPTIVE, kept (one uint32_t per slot) with RTW_ACCUM_FINITE.  A pointer the accumulator's flags
 * call for must be non-null and any other must be NULL, else RTW_ERR_INVALID_ARGUMENT.  The import checks `info`
 * and tile_stop as the older pairs do, and refuses a kept[slot] above the slot's sample count, or non-zero in a
 * padding slot, with a message naming kept.  The two older pairs refuse an accumulator with RTW_ACCUM_FINITE by
 * name (its state includes kept) and are otherwise unchanged.  Synchronous. */
RTW_API int rtw_accum_export_state(rtw_accum* a, float* host_sums, float* host_squares, uint32_t* host_tile_stop,
                                   uint32_t* host_kept);
RTW_API int rtw_accum_import_state(rtw_accum* a, const rtw_accum_info* info, const float* host_sums,
                                   const float* host_squares, const uint32_t* host_tile_stop, const uint32_t* host_kept);
/* RTW_ACCUM_CLAMP only (else RTW_ERR_INVALID_ARGUMENT).  rtw_accum_resolve_clamped: the clamped count of each pixel
 * or slot, laid out and padded as rtw_accum_resolve_kept.  rtw_accum_resolve_clamp_loss: lost / (float)kept per
 * channel (+0.0 for kept == 0), in the resolve's layout.  Asynchronous. */
RTW_API int rtw_accum_resolve_clamped(rtw_accum* a, uint32_t* d_out, void* stream);
RTW_API int rtw_accum_resolve_clamp_loss(rtw_accum* a, float* d_out, void* stream);
/* The checkpoint of an accumulator with RTW_ACCUM_CLAMP: the four arrays of rtw_accum_export_state, under its
 * must-be-non-null / must-be-NULL rule, plus clamped (one uint32_t per slot) and lost (3 * slots floats), both
 * non-null.  The import also refuses an `info` whose level (reserved) differs, a clamped[slot] above kept[slot],
 * and anything non-zero in a padding slot of clamped or lost, each with a message naming the field.  The three
 * older pairs refuse an accumulator with RTW_ACCUM_CLAMP by name and are otherwise unchanged.  Synchronous. */
RTW_API int rtw_accum_export_state_clamp(rtw_accum* a, float* host_sums, float* host_squares, uint32_t* host_tile_stop,
                                         uint32_t* host_kept, uint32_t* host_clamped, float* host_lost);
RTW_API int rtw_accum_import_state_clamp(rtw_accum* a, const rtw_accum_info* info, const float* host_sums,
                                         const float* host_squares, const uint32_t* host_tile_stop,
                                         const uint32_t* host_kept, const uint32_t* host_clamped, const float* host_lost);

/* ---- partition records: accumulators across GPUs ------------------------------------------- */
/* N accumulators of parts (0..N-1, N) of one frame, one per GPU, make the whole image's accumulator: each packs
 * its state into a record, the records are gathered onto one device (one collective), and one launch places them
 * into an accumulator of part (0, 1) there.  Sums, squares and kept are tile-major: local tile lt
 * of part (r, N) is tile r + lt * N of the frame, and part (0, 1) holds tile t at local index t, so the merge is a
 * placement of tile blocks.  Stop decisions are per tile and the RNG streams are keyed by (seed, pixel, sample):
 * the merged accumulator is, bit for bit, the one a single GPU would hold.
 *
 * The record, in 4-byte words (include/rtw_parts.h has the arithmetic; S0 and T0 are the slots and tiles of part
 * (0, N), which owns the most tiles, so all N records have one size and one set of section offsets):
 *   header     8 words: record version (1), flags (RTW_ACCUM_*), part_index, part_count, samples, slots, tiles, and
 *                       0 or, with RTW_ACCUM_CLAMP, the bits of the f32 level
 *   sums       3 * S0 f32
 *   squares    3 * S0 f32   with RTW_ACCUM_MOMENTS
 *   kept       S0 u32       with RTW_ACCUM_FINITE
 *   clamped    S0 u32       with RTW_ACCUM_CLAMP
 *   lost       3 * S0 f32   with RTW_ACCUM_CLAMP
 *   tile_stop  T0 u32       with RTW_ACCUM_ADAPTIVE
 * A section's words past the partition's own slots or tiles are zero.
 *
 * rtw_accum_packed_bytes: the bytes of one such record for params' frame (params' own part is not read) and
 * part_count parts.  Host only. */
RTW_API int rtw_accum_packed_bytes(const rtw_render_params* params, uint32_t flags, int32_t part_count, int64_t* bytes);
/* Copies the accumulator's state into the device buffer d_packed (4-byte aligned, rtw_accum_packed_bytes for the
 * accumulator's own part_count): header, sections, zeros in the tails.  Any accumulator, of any part and layout.
 * Ordered with the accumulator's other calls; asynchronous on `stream`. */
RTW_API int rtw_accum_pack(rtw_accum* a, void* d_packed, void* stream);
/* Replaces all of `whole`'s state by the merge of part_count records, record r at d_gathered + r * stride_bytes
 * (the shape rtw_untile_device takes; stride_bytes a multiple of 4, at least rtw_accum_packed_bytes).  `whole` is of
 * part (0, 1).  First the headers are read back, after the work already on `stream` and after the calls already
 * issued on whole's world (the packs of its other accumulators, on any stream), and refused with a message
 * naming the field: stride_bytes; a record's version, flags (against whole's), part_index (record r holds part r),
 * part_count, slots and tiles (against the arithmetic), reserved (with RTW_ACCUM_CLAMP: clamp, the level against
 * whole's); samples, which must be equal in all records
 * unless the flags hold RTW_ACCUM_ADAPTIVE.  With it whole's samples becomes the largest: rtw_accum_add does not
 * count when every tile of a part has stopped, so such a part's count stays where its last tile stopped, and the
 * largest is the count a single GPU would hold; its stop sections are read back too and a tile_stop of 1 or above
 * its record's samples is refused as rtw_accum_import_adaptive refuses it.  kept is not checked value by value: it
 * comes from accumulators, not from a file.  Nothing is launched or changed on a refusal.  Then one launch places
 * every record's tile blocks; whole may be read (resolve, stderr, noise, adapt, export) or added to as if it had
 * taken the samples itself.  The launch is asynchronous on `stream`; the call synchronizes it for the headers and,
 * adaptive, once more for the host's copy of the stop map.  The records themselves are only read. */
RTW_API int rtw_accum_merge_parts(rtw_accum* whole, const void* d_gathered, int64_t stride_bytes, int32_t part_count,
                                  void* stream);
/* The same merge on host arrays, without a GPU: `gathered` in the record layout above; sums and squares 3 * slots
 * floats and kept slots entries of the whole image (slots = tiles * tile_width * tile_height), tile_stop its tiles;
 * a pointer the flags call for is non-null and any other NULL.  *samples gets the merged count.  The same refusals;
 * nothing is written on one. */
RTW_API int rtw_accum_merge_parts_host(const rtw_render_params* params, uint32_t flags, const void* gathered,
                                       int64_t stride_bytes, int32_t part_count, float* sums, float* squares,
                                       uint32_t* kept, uint32_t* tile_stop, uint32_t* samples);
/* The same for records of accumulators with RTW_ACCUM_CLAMP (flags must hold it; rtw_accum_merge_parts_host refuses
 * such flags by name): `level` is the whole's, a record of another level is refused naming clamp; clamped slots
 * entries and lost 3 * slots floats of the whole image, both non-null. */
RTW_API int rtw_accum_merge_parts_host_clamp(const rtw_render_params* params, uint32_t flags, float level,
                                             const void* gathered, int64_t stride_bytes, int32_t part_count, float* sums,
                                             float* squares, uint32_t* kept, uint32_t* clamped, float* lost,
                                             uint32_t* tile_stop, uint32_t* samples);

/* ---- first-hit AOVs ------------------------------------------------------------------------- */
/* An AOV accumulator keeps, per pixel of the whole image, running sums of what the camera rays hit first:
 * albedo, normal and depth.  An AOV sample is one camera ray and one closest hit, no bounce;
 * it draws the (seed, pixel, sample) stream of the colour sample, so AOV sample s describes the primary ray of
 * colour sample s: same jitter, lens point, time and volume draws.  Per pixel pix = y * W + x and sample s:
 *   rng = rtw_sample_stream(rtw_seed_key(seed), pix, s); the two jitter draws; Camera::ray; the reference's
 *   closest hit over [0.001, inf) with the rng carried on.
 *   hit:  a = (1, 1, 1) for a dielectric, else 0 + 1 * the material's texture at the hit (every other kind, a
 *         DiffuseLight's emit texture included); nrm = (n + 1) * 0.5 (the RTW_MODE_NORMALS expression);
 *         depth_sum = depth_sum + t; hits += 1.
 *   miss: a = (1, 1, 1); nrm = the ray's background, as RTW_MODE_NORMALS gives it.
 *   sum = sum + value per channel, in sample order, from +0.
 * Resolve: albedo and normal sum / (float)samples; depth hits ? depth_sum / (float)hits : 0 (finite on a miss:
 * it can serve as a guide channel).  Adds of n1, n2, ... give the bits of one add of n1 + n2 + ...; the normal
 * image is bit-identical to a RTW_MODE_NORMALS frame of the same seed and samples_per_pixel; the albedo image
 * is the reference's radiance of the world's emissive twin (every material a DiffuseLight of its own texture,
 * a dielectric one of solid white, no light rect, background solid white, max_depth 2).
 *
 * rtw_aov_create reads width, height and seed from params, and refuses, naming the field: RTW_LAYOUT_TILES,
 * part_count > 1 and thread_count > 1 (RTW_ERR_UNSUPPORTED: the pass covers the whole image, in
 * RTW_LAYOUT_IMAGE); channels 0 or with an unknown bit and reserved0 != 0 (RTW_ERR_INVALID_ARGUMENT).  The
 * params are checked before the world, and nothing is allocated or launched for params it refuses.  The
 * accumulator owns its sums and touches none of the world's scratch: colour accumulators, one-shot frames and
 * AOV accumulators of one world interleave freely.  Calls on one AOV accumulator are ordered by the caller
 * (one stream, or events).  rtw_world_release takes its device state as it takes a colour accumulator's. */
#define RTW_AOV_ALBEDO 1u
#define RTW_AOV_NORMAL 2u
#define RTW_AOV_DEPTH 4u
typedef struct rtw_aov rtw_aov;
typedef struct rtw_aov_info { /* all fields fixed-width, no padding */
    uint32_t version;  /* 1 */
    uint32_t channels; /* RTW_AOV_* */
    int32_t width, height;
    uint32_t samples;  /* samples added so far, per pixel */
    uint32_t reserved; /* 0 */
    uint64_t seed;
    uint64_t world_fingerprint; /* rtw_world_fingerprint of the uploaded world */
} rtw_aov_info;
RTW_API int rtw_aov_create(rtw_gpu_world* gw, const rtw_render_params* params, uint32_t channels, rtw_aov** out);
RTW_API int rtw_aov_release(rtw_aov* a);
/* Traces samples [samples, samples + n) of every pixel and adds them.  Asynchronous on `stream`, one launch.
 * n == 0 does nothing; samples + n beyond 32 bits is RTW_ERR_INVALID_ARGUMENT. */
RTW_API int rtw_aov_add(rtw_aov* a, uint32_t n_samples, void* stream);
RTW_API int rtw_aov_get_info(rtw_aov* a, rtw_aov_info* out); /* host bookkeeping, no sync */
/* One channel (exactly one RTW_AOV_* bit) into device buffer d_out, RTW_LAYOUT_IMAGE: W*H*3 floats for albedo
 * and normal, W*H for depth.  RTW_ERR_INVALID_ARGUMENT for a channel the accumulator does not hold and at 0
 * samples.  Non-destructive, asynchronous. */
RTW_API int rtw_aov_resolve(rtw_aov* a, uint32_t channel, float* d_out, void* stream);
/* The samples of each pixel that hit something: W*H uint32_t.  Any accumulator, at any point.  Asynchronous. */
RTW_API int rtw_aov_hits(rtw_aov* a, uint32_t* d_out, void* stream);

/* ---- partitioned AOV accumulators: the AOV pass across GPUs --------------------------------- */
/* rtw_aov_create_part is rtw_aov_create for one partition of the frame: it reads part_index and
 * part_count (0 <= part_index < part_count; part_count 0 counts as 1) and takes RTW_LAYOUT_TILES as well as
 * RTW_LAYOUT_IMAGE (a part has no image of its own either way).  Part (r, N) owns the frame's 8 x 8 tiles
 * t = r, r + N, ..., the colour accumulators' partition: local tile lt is tile r + lt * N, slots is 64 times its
 * tile count and the planes are SoA over those slots.  Sample s of pixel p of a part is the whole image's (the
 * stream is keyed by (seed, pixel, sample); the leaf lists are the frame's, indexed by the frame's tile).  Part
 * (0, 1) is rtw_aov_create's accumulator exactly: same bits, same launches.  It refuses, naming the field, params
 * before the world, with nothing allocated: a tile other than 8 x 8 (tile_width / tile_height; 0 counts as 8: a
 * wave is a tile in this kernel), thread_count > 1 (RTW_ERR_UNSUPPORTED); an unknown layout, a bad part, and what
 * rtw_aov_create refuses of channels, reserved0 and the size (RTW_ERR_INVALID_ARGUMENT).  part_count may be above
 * the frame's tile count: such a part holds no tiles, and rtw_aov_add on it launches nothing and still counts
 * samples, so that the records of a group agree.  rtw_aov_resolve and rtw_aov_hits on an accumulator of
 * part_count > 1 return RTW_ERR_UNSUPPORTED naming part_count: a part is read through its state or after a merge.
 * Calls on one AOV accumulator (add, pack, merge, export, import, resolve) stay ordered by the caller: one
 * stream, or events. */
RTW_API int rtw_aov_create_part(rtw_gpu_world* gw, const rtw_render_params* params, uint32_t channels, rtw_aov** out);

/* The packed record of an AOV part, in 4-byte words (include/rtw_aov_parts.h has the arithmetic; S0 and T0 are the
 * slots and tiles of part (0, N), so all N records have one size):
 *   header   8 words: record version (1), channels, part_index, part_count, samples, slots, tiles, a non-zero magic
 *            (a colour record holds 0 there: each merge refuses the other's records by name)
 *   albedo 3 planes, normal 3 planes, depth 1 plane (each if held), hits 1 plane (always): S0 words each
 * A plane's words past the part's own slots are zero.
 *
 * rtw_aov_packed_bytes: the bytes of one such record for params' frame (params' own part is not read), the
 * channels and part_count parts.  Host only. */
RTW_API int rtw_aov_packed_bytes(const rtw_render_params* params, uint32_t channels, int32_t part_count, int64_t* bytes);
/* Copies the accumulator's planes into the device buffer d_packed (4-byte aligned, rtw_aov_packed_bytes for the
 * accumulator's own part_count): header, planes, zeros in the tails.  Any AOV accumulator, of any part.
 * Asynchronous on `stream`. */
RTW_API int rtw_aov_pack(rtw_aov* a, void* d_packed, void* stream);
/* Replaces all of `whole`'s planes by the merge of part_count records, record r at d_gathered + r * stride_bytes
 * (stride_bytes a multiple of 4, at least rtw_aov_packed_bytes).  `whole` is of part (0, 1).  First the headers are
 * read back, after the work already on `stream`, and refused with a message naming the field: stride_bytes; a
 * record's version, magic, channels (against whole's), part_index (record r holds part r), part_count, slots and
 * tiles (against the arithmetic); samples, which must be equal in all records.  Nothing is launched or changed on
 * a refusal.  Then one launch places every plane's tile blocks and whole's samples becomes the records' count:
 * whole may be resolved or added to as if it had traced the samples itself.  The launch is asynchronous on
 * `stream`; the call synchronizes it once for the headers.  The records themselves are only read. */
RTW_API int rtw_aov_merge_parts(rtw_aov* whole, const void* d_gathered, int64_t stride_bytes, int32_t part_count,
                                void* stream);
/* The same merge on host arrays, without a GPU: albedo and normal 3 planes of the whole image's slots
 * (tiles * 64) each, depth and hits one plane; albedo, normal and depth non-null exactly for a channel held.
 * *samples gets the records' count.  The same refusals; nothing is written on one. */
RTW_API int rtw_aov_merge_parts_host(const rtw_render_params* params, uint32_t channels, const void* gathered,
                                     int64_t stride_bytes, int32_t part_count, float* albedo, float* normal, float* depth,
                                     uint32_t* hits, uint32_t* samples);

/* The state of an AOV accumulator of any part: this header and its planes.  rtw_aov_info stays version 1. */
typedef struct rtw_aov_state_info { /* all fields fixed-width, no padding; also the checkpoint header */
    uint32_t version;  /* 1 */
    uint32_t channels; /* RTW_AOV_* */
    int32_t width, height;
    uint32_t samples;
    int32_t part_index, part_count;
    uint32_t slots; /* words of one plane: tiles * 64 */
    uint32_t tiles; /* the part's own tiles */
    uint32_t reserved; /* 0 */
    uint64_t seed;
    uint64_t world_fingerprint;
} rtw_aov_state_info;
RTW_API int rtw_aov_get_state_info(rtw_aov* a, rtw_aov_state_info* out); /* host bookkeeping, no sync */
/* Copies the planes to the host: albedo and normal 3 * slots floats (plane-major, as on the device), depth slots
 * floats, hits slots counts.  A pointer is non-null exactly for a channel held (hits always).  Padding slots of
 * edge tiles hold zeros.  Synchronous: it waits for the device, so for every add already issued. */
RTW_API int rtw_aov_export_state(rtw_aov* a, float* host_albedo, float* host_normal, float* host_depth, uint32_t* host_hits);
/* Sets the planes and the sample count from an exported state.  Refused with a message naming the field, with
 * nothing written: any field of `info` that differs from the accumulator's own (samples apart); a hits[slot] above
 * info->samples; a non-zero word in a padding slot (a slot of an edge tile outside the image) of any plane.
 * Synchronous. */
RTW_API int rtw_aov_import_state(rtw_aov* a, const rtw_aov_state_info* info, const float* host_albedo,
                                 const float* host_normal, const float* host_depth, const uint32_t* host_hits);

/* ---- ray queries: closest hit and occlusion for the caller's rays ---------------------------- */
/* What a ray of the caller's hits: a pick, a visibility or shadow test, a bake, a probe of one
 * bounce.  hits[i] is Scene::hit (hittable.rs:130-137) of ray i over [t_start, rays[i].t_end): the reference's
 * depth-first walk of the reference tree, ties included, with its f32 arithmetic -- t, position, normal (flipped
 * to oppose the ray, front_face telling which way), uv, front_face and material are the reference's bits.  leaf is
 * the index into rtw_world.leaves.  The direction need not be unit length (t is in units of it); time may be any
 * finite float: it moves Animation leaves and nothing else.  A miss gives leaf = material = -1, front_face = 0, t
 * the ray's own t_end (its bits) and +0.0 elsewhere.  albedo[i] (RTW_CAST_ALBEDO) is the AOV pass's value at that
 * hit: (1, 1, 1) on a miss and on a dielectric, else 0 + 1 * the material's texture at the hit.
 * A volume leaf draws its distance from a stream of the ray's own: ray i starts from
 * rtw_sample_stream(rtw_seed_key(seed), (uint32_t)i, stream).  A batch is reproducible, and a ray's answer depends
 * on its index and on nothing else in the batch (in a world without volume leaves, not on its index either).
 * out[i] of the occlusion calls is hits[i].leaf >= 0 of the closest-hit call with the same params: the same walk in
 * the same order, left at the first leaf that accepts (until then the range's end has not moved, so its steps and
 * draws are a prefix of the closest-hit walk's).
 *
 * Refused with RTW_ERR_INVALID_ARGUMENT and a message naming the field, the parameters before the world, with
 * nothing launched or written: null params, rays, hits or out; flags with an unknown bit (the occlusion calls know
 * none); reserved0 != 0; a t_start that is NaN or infinite; n < 0 or n > 2^31 - 1; albedo NULL with RTW_CAST_ALBEDO
 * or non-NULL without it; device rays or hits that are not 16-byte aligned (the kernel moves a ray as two and a
 * record as three 16-byte words); a NULL world; a world that rtw_world_release has taken (the library keeps the set
 * of live handles for this; a handle is an address, so a stale one reads as live again once a later
 * rtw_world_upload has been given the freed address: drop a handle when you release it).  n == 0 is RTW_OK with
 * nothing launched or written.  The rays' own values are device data and are not validated: the walk is bounded by
 * the tree, so a ray with NaN or infinite components returns like any other (what it returns is the f32
 * arithmetic's answer).
 * The calls use none of the world's scratch: they interleave freely with frames, colour accumulators and AOV
 * accumulators of the world.  The *_device calls are asynchronous on `stream`, one launch each; rtw_cast and
 * rtw_occluded take host arrays (any alignment), stage them and wait. */
typedef struct rtw_ray { /* 32 bytes */
    float origin[3];
    float time;
    float direction[3];
    float t_end; /* the range's end, exclusive; +inf for none */
} rtw_ray;
typedef struct rtw_hit { /* 48 bytes */
    float t;
    int32_t leaf; /* index into rtw_world.leaves, -1 on a miss */
    float position[3];
    float normal[3];
    float uv[2];
    int32_t front_face; /* 1: the ray met the outside of the surface */
    int32_t material;   /* index into rtw_world.materials, -1 on a miss */
} rtw_hit;
#define RTW_CAST_ALBEDO 1u
typedef struct rtw_cast_params {
    uint32_t flags;  /* RTW_CAST_* */
    float t_start;   /* the range's start, inclusive (the renderer's is 0.001) */
    uint64_t seed;   /* the volume leaves' streams */
    uint32_t stream;
    uint32_t reserved0; /* 0 */
} rtw_cast_params;
RTW_API int rtw_cast_device(rtw_gpu_world* gw, const rtw_cast_params* params, const rtw_ray* d_rays, int64_t n,
                            rtw_hit* d_hits, float* d_albedo /* n * 3 floats, iff RTW_CAST_ALBEDO */, void* stream);
RTW_API int rtw_occluded_device(rtw_gpu_world* gw, const rtw_cast_params* params, const rtw_ray* d_rays, int64_t n,
                                uint8_t* d_out /* n bytes, 1 or 0 */, void* stream);
RTW_API int rtw_cast(rtw_gpu_world* gw, const rtw_cast_params* params, const rtw_ray* rays, int64_t n, rtw_hit* hits,
                     float* albedo);
RTW_API int rtw_occluded(rtw_gpu_world* gw, const rtw_cast_params* params, const rtw_ray* rays, int64_t n, uint8_t* out);

/* ---- radiance queries: path-traced colour along the caller's rays ----------------------------- */
/* What colour arrives along a ray of the caller's: an irradiance or reflection probe, a light-map
 * bake, a camera model of the caller's own, a re-shoot of a frame's noisy rays.  Sample k of ray i is the
 * reference's ray_color (rendering.rs:19-71; RenderMode::ray_color for RTW_MODE_NORMALS) of that ray -- the whole
 * path with its materials, textures, volumes and light mixture, in the reference's f32 arithmetic, NaN included --
 * drawn from the stream rtw_sample_stream(rtw_seed_key(seed), first_ray + i, first_sample + k).  The one stream
 * serves the walk's volume draws and the shading's draws in ray_color's order.
 * Every segment, the first included, searches [0.001, +inf): the record's t_end is NOT read, so the rays of a cast
 * batch can be passed as they are.  The direction need not be unit length and is used as given (reflect, the
 * dielectric's cos_theta); the background's argument is dot((0, 1, 0), direction) of the caller's ray; time moves
 * Animation leaves and every scattered ray inherits it.  mode is RTW_MODE_DEFAULT (colours) or RTW_MODE_NORMALS;
 * max_depth is rtw_render_params' (any int32_t: below 2 a path ends at its first hit).
 * A sample's value depends on (seed, first_ray + i, first_sample + k) and the ray, and on nothing else in the batch
 * or the launch: a batch may be split by rays (first_ray) or by samples (first_sample) and resumed.
 * The reduction: mean[i] = sum / (float)samples per channel, sum from +0.0 over the ray's samples in sample order
 * (the frame's own expression).  With RTW_RADIANCE_FINITE it is rtw_finite.h's: the sum runs over the samples
 * rtw_finite_sample keeps, in order, mean[i] = rtw_finite_mean(sum, kept[i]) (+0.0 for kept 0) and kept[i] is
 * returned -- a probe on a triangle mesh is otherwise NaN wherever a sample met the reference's 0 / 0 pdf.
 *
 * Refused with RTW_ERR_INVALID_ARGUMENT and a message naming the field, the parameters before the world, with
 * nothing launched or written: null params or arrays; flags with an unknown bit (the samples call knows none); a
 * mode that is no render mode; samples == 0; n < 0 or n > 2^31 - 1; n * samples > 2^31 - 1; first_sample + samples
 * or first_ray + n past 2^32; kept NULL with RTW_RADIANCE_FINITE or non-NULL without it; device rays that are not
 * 16-byte aligned; a NULL or released world (as the ray queries above).  n == 0 is RTW_OK with nothing launched.
 * The rays' own values are device data and are not validated: every walk is bounded by the tree and every path by
 * max_depth, so a ray with NaN or infinite components returns like any other.
 * The calls use none of the world's scratch: they interleave freely with frames, accumulators and ray queries.
 * The *_device calls are asynchronous on `stream`, one launch each; rtw_radiance_resolve_device needs no world
 * and runs on the current device.  rtw_radiance takes host arrays (any alignment), stages them and waits: it goes
 * through the batch in chunks of rays against a fixed sample buffer of 256 MiB, chunk c with first_ray + its offset,
 * so its result is the unchunked one.  (Tests only: the environment variable RTW_RADIANCE_BUFFER_BYTES, read at
 * each call, replaces the 256 MiB, so that a handful of rays already goes through in several chunks; a chunk
 * holds at least one ray.  It changes no result.) */
#define RTW_RADIANCE_FINITE 1u
typedef struct rtw_radiance_params { /* 32 bytes */
    uint32_t flags;        /* RTW_RADIANCE_*: read by the resolve and the host call only */
    int32_t mode;          /* RTW_MODE_DEFAULT / RTW_MODE_NORMALS */
    int32_t max_depth;     /* as rtw_render_params' */
    uint32_t samples;      /* >= 1 */
    uint32_t first_sample;
    uint32_t first_ray;
    uint64_t seed;
} rtw_radiance_params;
/* d_colors[(i * samples + k) * 3 + c]: the per-sample radiance */
RTW_API int rtw_radiance_samples_device(rtw_gpu_world* gw, const rtw_radiance_params* params, const rtw_ray* d_rays, int64_t n,
                                        float* d_colors, void* stream);
/* d_mean n * 3 floats, d_kept n counts (iff RTW_RADIANCE_FINITE), from d_colors */
RTW_API int rtw_radiance_resolve_device(const rtw_radiance_params* params, const float* d_colors, int64_t n, float* d_mean,
                                        uint32_t* d_kept, void* stream);
RTW_API int rtw_radiance(rtw_gpu_world* gw, const rtw_radiance_params* params, const rtw_ray* rays, int64_t n, float* mean,
                         uint32_t* kept);
/* Tests and tools: the number of consecutive work items (samples) a wave of the radiance kernel owns. */
RTW_API int rtw_debug_radiance_items(void);

/* ---- preview denoiser ---------------------------------------------------------------------- */
/* A variance-guided a-trous filter for accumulator previews, built on nothing but images:
 * a colour image, the standard error of its channels (rtw_accum_resolve_stderr) and an optional guide of
 * 0..4 channels per pixel (a RTW_MODE_NORMALS frame, say), all RTW_LAYOUT_IMAGE.  The arithmetic is a fixed
 * f32 expression (include/rtw_denoise.h): the device kernels, rtw_denoise_host and a numpy restatement give
 * the same bits.  Pixels whose colour sum, variance or guide is not finite are left out: no other pixel reads
 * them and they pass through bit for bit.  A preview filter: the exact image stays rtw_accum_resolve's. */
typedef struct rtw_denoise_params {
    int32_t width, height;        /* >= 2 */
    int32_t iterations;           /* 1..6: level i taps at a step of 1 << i pixels */
    int32_t guide_channels;       /* 0..4 */
    float sigma_l, sigma_g;       /* > 0: luminance tolerance in standard deviations; guide distance cut-off */
    int32_t reserved0, reserved1; /* 0 */
} rtw_denoise_params;
typedef struct rtw_denoiser rtw_denoiser;
/* Allocates the scratch of a width x height filter on `device`: two record buffers and the guide buffer,
 * 48 bytes per pixel. */
RTW_API int rtw_denoiser_create(int device, int32_t width, int32_t height, rtw_denoiser** out);
RTW_API int rtw_denoiser_release(rtw_denoiser* d);
/* Runs the filter on device buffers: d_color and d_stderr W*H*3 floats, d_guide W*H*guide_channels floats
 * (NULL only when guide_channels is 0), d_out W*H*3 floats (may be d_color: the prep pass copies out of the
 * inputs first), d_out_variance W*H floats or NULL (the variance of each pixel's filtered luminance estimate,
 * NaN for pixels that were left out).  RTW_ERR_INVALID_ARGUMENT, with a message naming the field, for a size
 * other than the denoiser's, iterations outside 1..6, guide_channels outside 0..4, a non-positive or
 * non-finite sigma, non-zero reserved fields and null pointers.  Asynchronous. */
RTW_API int rtw_denoiser_run(rtw_denoiser* d, const rtw_denoise_params* params, const float* d_color,
                             const float* d_stderr, const float* d_guide, float* d_out, float* d_out_variance,
                             void* stream);
/* The same filter on host arrays, without a GPU (the same refusals, but any size >= 2 x 2). */
RTW_API int rtw_denoise_host(const rtw_denoise_params* params, const float* color, const float* std_err,
                             const float* guide, float* out, float* out_variance);
/* Albedo demodulation: the same calls plus an albedo image (W*H*3 floats, RTW_LAYOUT_IMAGE; a
 * resolved RTW_AOV_ALBEDO channel, say).  The filter runs on colour / D and standard error / D with
 * D_c = albedo_c >= 1/64 ? albedo_c : 1/64, and the output is the filtered value times D: a texture's contrast
 * is divided out before the filter compares neighbours and put back after it (include/rtw_denoise.h has the
 * order).  A pixel with a non-finite albedo channel is left out like one with a non-finite guide, and every
 * pixel that is left out returns its input colour bit for bit.  The variance output is that of the
 * demodulated luminance estimate, (r/D_r + g/D_g) + b/D_b.  albedo == NULL: exactly the calls above. */
RTW_API int rtw_denoiser_run_albedo(rtw_denoiser* d, const rtw_denoise_params* params, const float* d_color,
                                    const float* d_stderr, const float* d_guide, const float* d_albedo, float* d_out,
                                    float* d_out_variance, void* stream);
RTW_API int rtw_denoise_host_albedo(const rtw_denoise_params* params, const float* color, const float* std_err,
                                    const float* guide, const float* albedo, float* out, float* out_variance);

/* Floats needed by one partition's RTW_LAYOUT_TILES buffer (tiles * tile_w * tile_h * 3). */
RTW_API int rtw_partition_floats(const rtw_render_params* params, int64_t* floats);
/* Scatters part_count gathered tile buffers (each padded to `stride_floats`) into a W*H*3
 * image on the device (rank 0 after the RCCL gather). */
RTW_API int rtw_untile_device(const rtw_render_params* params, const float* d_tiles,
                              int64_t stride_floats, float* d_image, void* stream);
/* Synchronous statistics render (counting variant of the kernel): the reference's traversal
 * (hittable.rs:429-473 DFS over the reference BVH, with the proximity cull). */
RTW_API int rtw_render_collect_stats(rtw_gpu_world* gw, const rtw_render_params* params,
                                     rtw_render_stats* stats);
/* The same counts for the traversal the product kernel runs (tree 1): on worlds that take the SAH
 * walk, its node and leaf visits plus the leaf-box proof and the re-traced rays; elsewhere as
 * tree 0 (= rtw_render_collect_stats).  Approximate where the product kernel uses its wave-
 * cooperative trace: the counting variant re-traces tied rays on the reference tree and
 * walks the drain's last rays instead.  No reference counterpart: feeds the measured record bytes. */
RTW_API int rtw_render_collect_stats_tree(rtw_gpu_world* gw, const rtw_render_params* params, int tree,
                                          rtw_render_stats* stats);
/* Profiling aid (no reference counterpart): the statistics render plus up to n wave-level
 * execution counters of the kernel, in this order: traversal calls, traversal loop iterations,
 * iterations that ran the node step, iterations that ran the leaf step, lane node steps, lane
 * leaf steps, live lanes and lanes waiting for shading (summed over iterations), lanes whose
 * node passed, iterations / lanes testing an inline near sphere child, the same for the far
 * child, shade calls, lanes shaded, wave cycles in traversal, wave cycles elsewhere (refill,
 * ray setup, shading). */
#define RTW_DEBUG_COUNTERS 17
RTW_API int rtw_render_debug_counters(rtw_gpu_world* gw, const rtw_render_params* params,
                                      rtw_render_stats* stats, uint64_t* counters, int n);
/* Output encoder (color.rs:43-48 to_rgb8_gamma2), on the device: d_rgb8 gets W*H*3 bytes. */
RTW_API int rtw_encode_rgb8_device(const float* d_image, int64_t pixels, uint8_t* d_rgb8,
                                   void* stream);

/* Device self-test of the shared scalar spec (rtw_scalar.h): evaluates function `fn` on n
 * inputs on the device; 0 acos, 1 atan2, 2 ln, 3 sin, 4 div, 5 sqrt, 6 rcp-refined div. */
RTW_API int rtw_device_eval_scalar(int device, int fn, const float* a, const float* b, int64_t n,
                                   float* out);

/* Device self-test of the traversal's node step (Aabb::hit_cond, aabb.rs:65-78, AND the proximity
 * cull): for each i, box[6i..] = min xyz, max xyz; ray[6i..] = origin xyz, direction xyz;
 * range[2i..] = t_start, t_end; km[2i..] = the node's cull constants; mk_world as computed at upload
 * (1: node coordinates admit the per-ray exact-division guard).  out[i] = 1 if the node passes.
 * mk_world = 2 evaluates the SAH walk's node test instead (one-multiply quotients,
 * constants widened x17/16 as uploaded) beside the cull alone with exact quotients: out[i] bit 0 =
 * SAH test passes, bit 1 = exact cull passes, bit 2 = the ray admits the exact division.
 * mk_world = 3: the same with the D^2 k term the render kernel uses (2: round 2's Dq form). */
RTW_API int rtw_device_eval_node_pass(int device, const float* box, const float* ray, const float* range,
                                      const float* km, int32_t mk_world, int64_t n, int32_t* out);

/* Device self-test of CheckerTexture's sign test (texture.rs:33-40) as the render kernel evaluates
 * it: out[i] = 1 if RN(RN(sinf(x) sinf(y)) sinf(z)) < 0 for (x, y, z) = xyz[3i..3i+2], else 0. */
RTW_API int rtw_device_eval_checker(int device, const float* xyz, int64_t n, int32_t* out);

/* Device self-check of the exact fast divisions of the render kernel, counted on
 * the device over n cases: test 0 the refined hardware reciprocal against 1/b for b = bits(base + i);
 * test 1 division by pi and tau for a = bits(base + i); test 2 Markstein's correction on random
 * pairs inside its guards; test 3 the guarded division helpers on random pairs of any kind (zeros,
 * subnormals, extremes, infinities, NaN).  *mismatches = cases whose bits differ from IEEE division
 * (NaN = NaN), *first = the first such i (~0 if none). */
RTW_API int rtw_device_check_division(int device, int test, uint64_t base, uint64_t n, uint64_t seed,
                                      uint64_t* mismatches, uint64_t* first);

/* ---- host scene construction ------------------------------------------------------------- */
typedef struct rtw_builder rtw_builder;         /* WorldBuilder + arena (world_builder.rs:7-14) */
typedef struct rtw_world_handle rtw_world_handle; /* owns a finished flat World */
typedef struct rtw_rng rtw_rng;                 /* TRng = Xoroshiro128PlusPlus (common.rs:1) */

RTW_API rtw_rng* rtw_rng_from_seed(const uint8_t seed[16]);
RTW_API void rtw_rng_free(rtw_rng* rng);
RTW_API float rtw_rng_gen_f32(rtw_rng* rng);
RTW_API uint64_t rtw_rng_next_u64(rtw_rng* rng);

RTW_API rtw_builder* rtw_builder_new(void);
RTW_API void rtw_builder_free(rtw_builder* b);
/* Textures / materials return an id >= 0, or -1 on error (see rtw_last_error). */
RTW_API int32_t rtw_texture_solid(rtw_builder* b, float r, float g, float bl);
RTW_API int32_t rtw_texture_checker(rtw_builder* b, float inv_frequency, int32_t even,
                                    int32_t odd);
RTW_API int32_t rtw_texture_marble(rtw_builder* b, float scale, rtw_rng* rng);
RTW_API int32_t rtw_texture_image_rgb8(rtw_builder* b, const uint8_t* rgb, int32_t width,
                                       int32_t height);
RTW_API int32_t rtw_material_lambert(rtw_builder* b, int32_t albedo);
RTW_API int32_t rtw_material_metal(rtw_builder* b, int32_t albedo, float fuzz);
RTW_API int32_t rtw_material_dielectric(rtw_builder* b, float index_of_refraction);
RTW_API int32_t rtw_material_diffuse_light(rtw_builder* b, int32_t emit);
RTW_API int32_t rtw_material_isotropic(rtw_builder* b, int32_t albedo);
/* Nodes (world_builder.rs:104-270). */
RTW_API int32_t rtw_node_group(rtw_builder* b);
RTW_API int32_t rtw_node_sphere(rtw_builder* b, float radius, int32_t material);
RTW_API int32_t rtw_node_rect(rtw_builder* b, int32_t plane, const float center[3], float size0,
                              float size1, int32_t material);
RTW_API int32_t rtw_node_box(rtw_builder* b, float width, float height, float depth,
                             int32_t material);
/* triangles: n records of 24 floats (positions[3][3], normals[3][3], uvs[3][2]) */
RTW_API int32_t rtw_node_mesh(rtw_builder* b, const float* triangles, int32_t n,
                              int32_t material);
RTW_API int rtw_node_add(rtw_builder* b, int32_t parent, int32_t child);
RTW_API int rtw_node_translate(rtw_builder* b, int32_t node, float x, float y, float z);
RTW_API int rtw_node_rotate_around_up(rtw_builder* b, int32_t node, float degrees);
RTW_API int rtw_node_animate_moving(rtw_builder* b, int32_t node, float x, float y, float z);
RTW_API int rtw_node_set_all_geo_as_poi(rtw_builder* b, int32_t node);
RTW_API int rtw_node_set_all_geo_density(rtw_builder* b, int32_t node, float density);

/* Camera builder (camera.rs:11-152).  fov_mode 1: vertical_fov(a, b); 0: viewport(a, b).
 * look_mode 0: orientation(up, target=forward); 1: look_at(up, target); 2: look_at_focus. */
typedef struct rtw_camera_spec {
    int32_t fov_mode;
    float fov_a, fov_b;
    float position[3];
    int32_t look_mode;
    float up[3];
    float target[3];
    int32_t has_focus_distance;
    float focus_distance;
    int32_t has_focus_point;
    float focus_point[3];
    float aperture;
    float time0, time1;
} rtw_camera_spec;
RTW_API int rtw_camera_build(const rtw_camera_spec* spec, rtw_camera* out);
RTW_API float rtw_camera_aspect_ratio(const rtw_camera* cam); /* camera.rs:171-173 */

/* NodeRef::finish (world_builder.rs:273-290): flatten + one BVH over camera.time_interval. */
RTW_API int rtw_builder_finish(rtw_builder* b, int32_t root, const rtw_background* background,
                               const rtw_camera* camera, rtw_world_handle** out);
RTW_API const rtw_world* rtw_world_get(const rtw_world_handle* h);
RTW_API void rtw_world_free(rtw_world_handle* h);

/* obj_loader.rs:7-22 load_obj_mesh, fan-triangulation quirk included.  Returns n triangles as
 * n*24 floats in *out (free with rtw_free). */
RTW_API int rtw_obj_parse(const char* text, size_t len, float** out, int32_t* n);
RTW_API void rtw_free(void* p);

/* Demo worlds (demo_worlds.rs) seeded like main.rs:24.  `name` is "final_scene1",
 * "final_scene2", "cornell_box", "cornell_box_smoke", "cornell_cube", "suzanne",
 * "earth_mapped", "earth_motion", "moving_spheres", "perlin_spheres", "simple_plane",
 * "defocus_blur".  Meshes / images the world needs come in `assets`. */
typedef struct rtw_assets {
    const float* suzanne_tris; /* n*24 floats, from rtw_obj_parse */
    int32_t suzanne_count;
    const float* cube_tris;
    int32_t cube_count;
    const uint8_t* earth_rgb; /* RGB8, row 0 = top */
    int32_t earth_width, earth_height;
} rtw_assets;
RTW_API int rtw_demo_world(const char* name, const rtw_assets* assets, rtw_world_handle** out);

#ifdef __cplusplus
}
#endif

#endif /* RTW_H */

/* Containment check of the primary rays' per-tile leaf lists (include/rtw_beam.h, DESIGN.md 5.2
 * step 5).  Reads a world's camera and plain-sphere leaf records from a file, builds every tile's list
 * with the cap at the leaf count (so no tile may fall back to the walk), and for each tile draws
 * camera rays with a host restatement of camera_ray (camera.rs:175-200; csrc/rtw_device.hip) --
 * `rays` random ones, plus the extremes: jitter 0 and the largest jitter below the upper bound at all
 * four corner pixels, with lens points on the rim in 16 directions -- and runs the reference's f32
 * sphere test (sphere_geometry.rs:21-59) on every leaf with t_range [0.001, inf).  Every accepting
 * leaf must be in the tile's list.  Exit status 1 on any violation or any tile without a list.
 *   beam_lists_check FILE W H TW TH [RAYS]
 * FILE: 23 floats (rtw_camera), int32 n, 4 n floats ({c, r} per leaf).
 * Built with -ffp-contract=off like the kernel. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rtw_beam.h"

static uint64_t s = 0x9E3779B97F4A7C15ull;
static inline uint64_t nxt(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }

typedef struct { float e[3]; } V;
static V ld(const float* p) { V r = {{p[0], p[1], p[2]}}; return r; }
static V sub(V a, V b) { V r = {{a.e[0] - b.e[0], a.e[1] - b.e[1], a.e[2] - b.e[2]}}; return r; }
static V add(V a, V b) { V r = {{a.e[0] + b.e[0], a.e[1] + b.e[1], a.e[2] + b.e[2]}}; return r; }
static V mul(V a, float k) { V r = {{a.e[0] * k, a.e[1] * k, a.e[2] * k}}; return r; }
static float dot(V a, V b) { return (a.e[0] * b.e[0] + a.e[1] * b.e[1]) + a.e[2] * b.e[2]; }
static V unit(V a) { return mul(a, 1.0f / sqrtf(dot(a, a))); } /* vec3.rs unit(): v * (1/len) */

static int sphere_hit(V c, float r, V o, V d, float ts, float te) {
    const V oc = sub(o, c);
    const float hb = dot(oc, d);
    const float cc = dot(oc, oc) - r * r;
    const float disc = hb * hb - cc;
    if (disc < 0.0f) return 0;
    const float sq = sqrtf(disc);
    const float rs = -hb - sq;
    if (ts <= rs && rs < te) return 1;
    const float rl = -hb + sq;
    if (ts <= rl && rl < te) return 1;
    return 0;
}

/* camera_ray with the lens point (d0, d1) given */
static void camera_ray(const rtw_camera* c, float d0, float d1, float px, float py, V* o, V* d) {
    V off = {{0.0f, 0.0f, 0.0f}};
    if (c->lens_radius > 0.0f) off = mul(add(mul(ld(c->unit_right), d0), mul(ld(c->unit_up), d1)), c->lens_radius);
    *o = add(ld(c->position), off);
    *d = unit(sub(sub(add(ld(c->upper_left_corner), mul(ld(c->scaled_right), px)), mul(ld(c->scaled_up), py)), off));
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: %s FILE W H TW TH [RAYS]\n", argv[0]); return 2; }
    const int W = atoi(argv[2]), H = atoi(argv[3]), tw = atoi(argv[4]), th = atoi(argv[5]);
    const int rays = argc > 6 ? atoi(argv[6]) : 256;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    rtw_camera cam;
    int32_t n = 0;
    if (sizeof(cam) != 23 * sizeof(float) || fread(&cam, sizeof(cam), 1, f) != 1 || fread(&n, 4, 1, f) != 1 || n < 1 ||
        W < 2 || H < 2 || tw < 1 || th < 1) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    float* fast = (float*)malloc((size_t)n * 4 * sizeof(float));
    int32_t* list = (int32_t*)malloc((size_t)n * sizeof(int32_t));
    unsigned char* in = (unsigned char*)malloc((size_t)n);
    if (!fast || !list || !in || fread(fast, 4 * sizeof(float), (size_t)n, f) != (size_t)n) { fprintf(stderr, "bad input\n"); return 2; }
    fclose(f);

    const float inf = rtw_u2f(0x7F800000u);
    const float sx = 1.0f / (float)(W - 1), sy = 1.0f / (float)(H - 1);
    const rtw_uniform ux = rtw_uniform_new(0.0f, sx), uy = rtw_uniform_new(0.0f, sy); /* the kernel's jitter */
    const float vmax = rtw_u2f((0xFFFFFFFFu >> 9) | 0x3F800000u) - 1.0f;               /* the largest value0_1 */
    const int tiles_x = (W + tw - 1) / tw, tiles_y = (H + th - 1) / th;
    long empty = 0, listed = 0, walked = 0, entries = 0, violations = 0, tested = 0, accepted = 0;
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) {
            const int32_t cnt = rtw_beam_tile_list(&cam, W, H, tw, th, tx, ty, fast, n, n, list);
            if (cnt < 0) { ++walked; continue; }
            if (cnt == 0) ++empty; else ++listed;
            entries += cnt;
            memset(in, 0, (size_t)n);
            for (int j = 0; j < cnt; ++j) in[list[j]] = 1;
            const int x0 = tx * tw, y0 = ty * th;
            const int x1 = (x0 + tw - 1 < W - 1) ? x0 + tw - 1 : W - 1, y1 = (y0 + th - 1 < H - 1) ? y0 + th - 1 : H - 1;
            const int extremes = 4 * 4 * 16; /* corner pixel x jitter corner x rim direction */
            for (int q = 0; q < rays + extremes; ++q) {
                int x, y;
                float vx, vy, d0, d1;
                if (q < rays) {
                    x = x0 + (int)(nxt() % (uint64_t)(x1 - x0 + 1));
                    y = y0 + (int)(nxt() % (uint64_t)(y1 - y0 + 1));
                    vx = rtw_value0_1((uint32_t)nxt());
                    vy = rtw_value0_1((uint32_t)nxt());
                    do { /* UnitDisc: rejection from the square, <= 1 accepted */
                        d0 = rtw_value0_1((uint32_t)nxt()) * 2.0f - 1.0f;
                        d1 = rtw_value0_1((uint32_t)nxt()) * 2.0f - 1.0f;
                    } while (!(d0 * d0 + d1 * d1 <= 1.0f));
                } else {
                    const int e = q - rays, cp = e / 64, cj = (e / 16) % 4, dir = e % 16;
                    x = (cp & 1) ? x1 : x0;
                    y = (cp & 2) ? y1 : y0;
                    vx = (cj & 1) ? vmax : 0.0f;
                    vy = (cj & 2) ? vmax : 0.0f;
                    const double a = 2.0 * 3.14159265358979323846 * dir / 16.0;
                    d0 = (float)cos(a);
                    d1 = (float)sin(a);
                    while (!(d0 * d0 + d1 * d1 <= 1.0f)) { d0 *= 1.0f - 0x1p-23f; d1 *= 1.0f - 0x1p-23f; }
                }
                const float px = (float)x * sx + (vx * ux.scale + ux.low), py = (float)y * sy + (vy * uy.scale + uy.low);
                V o, d;
                camera_ray(&cam, d0, d1, px, py, &o, &d);
                for (int i = 0; i < n; ++i) {
                    ++tested;
                    if (!sphere_hit(ld(fast + 4 * i), fast[4 * i + 3], o, d, 0.001f, inf)) continue;
                    ++accepted;
                    if (!in[i]) {
                        if (violations < 10) printf("VIOLATION tile (%d, %d) pixel (%d, %d) leaf %d not listed\n", tx, ty, x, y, i);
                        ++violations;
                    }
                }
            }
        }
    const long tiles = (long)tiles_x * tiles_y;
    printf("tiles %ld listed %ld empty %ld walked %ld leaves %d mean_len %.4f tests %ld accepted %ld violations %ld\n", tiles,
           listed, empty, walked, n, (listed + empty) ? (double)entries / (double)(listed + empty) : 0.0, tested, accepted,
           violations);
    free(fast);
    free(list);
    free(in);
    return violations != 0 || walked != 0;
}

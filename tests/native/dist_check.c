/* dist_check.c -- raw moments and histograms of the shared spec's samplers (include/rtw_scalar.h), stand-alone
 * (tests/test_distributions.py builds it with gcc, runs it and compares the figures with the closed forms).
 *
 *   dist_check <threads>
 *
 * Every sampler draws 2^26 values: 64 xoroshiro streams of 2^20 draws each, seeded from the stream's number alone
 * (so the figures do not depend on the thread count), the streams shared out over the threads.  Per sampler the
 * lines `<sampler>.n`, `.counts` (4 integers), `.sums` (12 f64 sums, %.17g), `.hist0` and `.hist1` (64 bins each):
 *
 *   gen_f32        counts: off the 2^-24 grid, outside [0, 1) | sums: v, v^2 | hist0 of [0, 1)
 *   uniform        rtw_uniform_sample of Uniform::new(0, 1/47).  counts: outside [0, high) | sums: v, v^2 | hist0
 *   range          rtw_gen_range_f32(-1, 3).  counts: outside [-1, 3) | sums: v, v^2 | hist0
 *   tight          the range [100, 101), where scale * max + low rounds up to high.  counts: 1 if it does, the
 *                  Uniform's draws outside the range, gen_range's | sums: the Uniform's v, gen_range's
 *   bool           counts: true
 *   u32_3, u32_7   counts: out of range | hist0: the count of each value
 *   u32_big        rtw_gen_range_u32(2^31 + 1).  counts: out of range | hist0 of value * 64 / (2^31 + 1)
 *   disc           counts: r^2 > 1 + 2^-22 | sums: x, y, x^2, y^2, xy | hist0 of r^2 | hist1 of the angle
 *   sphere         sums: x, y, z, x^2, y^2, z^2, xy, xz, yz, max | |p| - 1 | | hist0 of z | hist1 of x
 *   ball           counts: r^2 > 1 + 2^-22 | sums: x, y, z | hist0 of r^3 | hist1 of z
 *   lobe_z,        unit(n + unit_sphere) in f32, as the oracle's dist_generate, about n = (0, 0, 1) and about
 *   lobe_tilted    n = (2, -1, 2) / 3.  counts: cos <= 0 | sums: cos | hist0 of cos^2
 */
#include <inttypes.h>
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rtw_scalar.h"

#define STREAMS 64
#define DRAWS (1u << 20)
#define BINS 64
#define PI 3.14159265358979323846

typedef struct Acc {
    double s[12];
    uint64_t c[4];
    uint64_t h[2][BINS];
} Acc;

enum { D_F32, D_UNIFORM, D_RANGE, D_TIGHT, D_BOOL, D_U3, D_U7, D_UBIG, D_DISC, D_SPHERE, D_BALL, D_LOBE0, D_LOBE1, D_COUNT };
static const char* NAMES[D_COUNT] = {"gen_f32", "uniform", "range", "tight", "bool", "u32_3", "u32_7", "u32_big",
                                     "disc", "sphere", "ball", "lobe_z", "lobe_tilted"};
static Acc acc[STREAMS][D_COUNT];
static int next_stream;
static pthread_mutex_t lock = PTHREAD_MUTEX_INITIALIZER;

static rtw_xoro stream_rng(int stream, int dist) {
    uint64_t x = 0x243F6A8885A308D3ull ^ ((uint64_t)stream << 32) ^ (uint64_t)dist;
    rtw_xoro r;
    r.s0 = rtw_splitmix64_next(&x);
    r.s1 = rtw_splitmix64_next(&x);
    return r;
}

static int bin_of(double v, double lo, double hi) {
    int b = (int)floor((v - lo) / (hi - lo) * BINS);
    return b < 0 ? 0 : (b >= BINS ? BINS - 1 : b);
}

static void lobe(Acc* a, rtw_xoro* r, const float n[3]) {
    for (uint32_t i = 0; i < DRAWS; ++i) {
        float s[3];
        rtw_unit_sphere(r, s);
        const float v[3] = {n[0] + s[0], n[1] + s[1], n[2] + s[2]};
        const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!(len > 0.0f)) { a->c[0]++; continue; }
        const float d[3] = {v[0] / len, v[1] / len, v[2] / len};
        const double c = (double)n[0] * d[0] + (double)n[1] * d[1] + (double)n[2] * d[2];
        if (!(c > 0.0)) a->c[0]++;
        a->s[0] += c;
        a->h[0][bin_of(c * c, 0.0, 1.0)]++;
    }
}

static void run(int stream, int dist) {
    Acc* a = &acc[stream][dist];
    rtw_xoro r = stream_rng(stream, dist);
    switch (dist) {
        case D_F32:
            for (uint32_t i = 0; i < DRAWS; ++i) {
                const float v = rtw_gen_f32(&r);
                const double d = v, g = d * 16777216.0;
                a->s[0] += d; a->s[1] += d * d;
                if (g != floor(g)) a->c[0]++;
                if (!(v < 1.0f) || v < 0.0f) a->c[1]++;
                a->h[0][bin_of(d, 0.0, 1.0)]++;
            }
            break;
        case D_UNIFORM: {
            const float high = 1.0f / 47.0f;
            const rtw_uniform u = rtw_uniform_new(0.0f, high);
            for (uint32_t i = 0; i < DRAWS; ++i) {
                const float v = rtw_uniform_sample(&u, &r);
                a->s[0] += v; a->s[1] += (double)v * v;
                if (!(v < high) || v < 0.0f) a->c[0]++;
                a->h[0][bin_of(v, 0.0, high)]++;
            }
            break;
        }
        case D_RANGE:
            for (uint32_t i = 0; i < DRAWS; ++i) {
                const float v = rtw_gen_range_f32(-1.0f, 3.0f, &r);
                a->s[0] += v; a->s[1] += (double)v * v;
                if (!(v < 3.0f) || v < -1.0f) a->c[0]++;
                a->h[0][bin_of(v, -1.0, 3.0)]++;
            }
            break;
        case D_TIGHT: {
            const float low = 100.0f, high = 101.0f;
            const float max_rand = rtw_u2f((0xFFFFFFFFu >> 9) | 0x3F800000u) - 1.0f;
            const volatile float top = (high - low) * max_rand + low;
            a->c[0] = top >= high;
            const rtw_uniform u = rtw_uniform_new(low, high);
            for (uint32_t i = 0; i < DRAWS; ++i) {
                const float v = rtw_uniform_sample(&u, &r);
                const float w = rtw_gen_range_f32(low, high, &r);
                if (!(v < high) || v < low) a->c[1]++;
                if (!(w < high) || w < low) a->c[2]++;
                a->s[0] += v; a->s[1] += w;
            }
            break;
        }
        case D_BOOL:
            for (uint32_t i = 0; i < DRAWS; ++i) a->c[0] += (uint64_t)(rtw_gen_bool_half(&r) != 0);
            break;
        case D_U3:
        case D_U7: {
            const uint32_t n = dist == D_U3 ? 3u : 7u;
            for (uint32_t i = 0; i < DRAWS; ++i) {
                const uint32_t v = rtw_gen_range_u32(n, &r);
                if (v >= n) a->c[0]++; else a->h[0][v]++;
            }
            break;
        }
        case D_UBIG: {
            const uint32_t n = 0x80000001u;
            for (uint32_t i = 0; i < DRAWS; ++i) {
                const uint32_t v = rtw_gen_range_u32(n, &r);
                if (v >= n) a->c[0]++; else a->h[0][(uint32_t)(((uint64_t)v * BINS) / n)]++;
            }
            break;
        }
        case D_DISC:
            for (uint32_t i = 0; i < DRAWS; ++i) {
                float p[2];
                rtw_unit_disc(&r, p);
                const double x = p[0], y = p[1], r2 = x * x + y * y;
                if (r2 > 1.0 + 0x1p-22) a->c[0]++;
                a->s[0] += x; a->s[1] += y; a->s[2] += x * x; a->s[3] += y * y; a->s[4] += x * y;
                a->h[0][bin_of(r2, 0.0, 1.0)]++;
                a->h[1][bin_of(atan2(y, x), -PI, PI)]++;
            }
            break;
        case D_SPHERE:
            for (uint32_t i = 0; i < DRAWS; ++i) {
                float p[3];
                rtw_unit_sphere(&r, p);
                const double x = p[0], y = p[1], z = p[2], e = fabs(sqrt(x * x + y * y + z * z) - 1.0);
                if (e > a->s[9]) a->s[9] = e;
                a->s[0] += x; a->s[1] += y; a->s[2] += z;
                a->s[3] += x * x; a->s[4] += y * y; a->s[5] += z * z;
                a->s[6] += x * y; a->s[7] += x * z; a->s[8] += y * z;
                a->h[0][bin_of(z, -1.0, 1.0)]++;
                a->h[1][bin_of(x, -1.0, 1.0)]++;
            }
            break;
        case D_BALL:
            for (uint32_t i = 0; i < DRAWS; ++i) {
                float p[3];
                rtw_unit_ball(&r, p);
                const double x = p[0], y = p[1], z = p[2], r2 = x * x + y * y + z * z;
                if (r2 > 1.0 + 0x1p-22) a->c[0]++;
                a->s[0] += x; a->s[1] += y; a->s[2] += z;
                a->h[0][bin_of(r2 * sqrt(r2), 0.0, 1.0)]++;
                a->h[1][bin_of(z, -1.0, 1.0)]++;
            }
            break;
        case D_LOBE0: {
            const float n[3] = {0.0f, 0.0f, 1.0f};
            lobe(a, &r, n);
            break;
        }
        default: {
            const float n[3] = {2.0f / 3.0f, -1.0f / 3.0f, 2.0f / 3.0f};
            lobe(a, &r, n);
            break;
        }
    }
}

static void* worker(void* arg) {
    (void)arg;
    for (;;) {
        pthread_mutex_lock(&lock);
        const int job = next_stream++;
        pthread_mutex_unlock(&lock);
        if (job >= STREAMS * D_COUNT) return NULL;
        run(job / D_COUNT, job % D_COUNT);
    }
}

static void print_hist(const char* name, const char* what, const Acc* t, int k, int bins) {
    printf("%s.%s", name, what);
    for (int b = 0; b < bins; ++b) printf(" %" PRIu64, t->h[k][b]);
    printf("\n");
}

int main(int argc, char** argv) {
    int threads = argc > 1 ? atoi(argv[1]) : 1;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    pthread_t th[64];
    for (int t = 0; t < threads; ++t) pthread_create(&th[t], NULL, worker, NULL);
    for (int t = 0; t < threads; ++t) pthread_join(th[t], NULL);
    for (int d = 0; d < D_COUNT; ++d) {
        Acc t;
        memset(&t, 0, sizeof(t));
        for (int s = 0; s < STREAMS; ++s) { /* in stream order: the sums do not depend on the thread count */
            const Acc* a = &acc[s][d];
            for (int i = 0; i < 12; ++i) {
                if (d == D_SPHERE && i == 9) { if (a->s[i] > t.s[i]) t.s[i] = a->s[i]; }
                else t.s[i] += a->s[i];
            }
            for (int i = 0; i < 4; ++i) {
                if (d == D_TIGHT && i == 0) t.c[i] = a->c[i];
                else t.c[i] += a->c[i];
            }
            for (int k = 0; k < 2; ++k)
                for (int b = 0; b < BINS; ++b) t.h[k][b] += a->h[k][b];
        }
        const char* nm = NAMES[d];
        printf("%s.n %" PRIu64 "\n", nm, (uint64_t)STREAMS * DRAWS);
        printf("%s.counts %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", nm, t.c[0], t.c[1], t.c[2], t.c[3]);
        printf("%s.sums", nm);
        for (int i = 0; i < 12; ++i) printf(" %.17g", t.s[i]);
        printf("\n");
        print_hist(nm, "hist0", &t, 0, BINS);
        print_hist(nm, "hist1", &t, 1, BINS);
    }
    return 0;
}

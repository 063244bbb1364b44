/* The adaptive accumulator's tile test on the host (include/rtw_adapt.h): rtw_adapt_tiles, the header
 * function behind librtw.so's rtw_adapt_tiles_host, run stand-alone so that a sanitizer build can watch
 * every index it forms.
 *   adapt_check FILE
 * FILE: int32 width, height, tile_w, tile_h, part_index, part_count; uint32 samples, min_samples;
 * float target; int32 tiles; then 3 * tiles * tile_w * tile_h floats of sums, as many of squares, and
 * `tiles` uint32 of the stop map before the call.  The arrays are copied into exact-size heap blocks.
 * Prints "rc R tiles T" and the stop map after the call, one entry per line.  Exit status 2 on a short or
 * inconsistent file.  Built with -ffp-contract=off like the kernel. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rtw_adapt.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t g[6];
    uint32_t u[2];
    float target;
    int32_t tiles;
    if (fread(g, 4, 6, f) != 6 || fread(u, 4, 2, f) != 2 || fread(&target, 4, 1, f) != 1 || fread(&tiles, 4, 1, f) != 1) return 2;
    rtw_render_params p;
    memset(&p, 0, sizeof(p));
    p.width = g[0];
    p.height = g[1];
    p.tile_width = g[2];
    p.tile_height = g[3];
    p.part_index = g[4];
    p.part_count = g[5];
    rtw_adapt_geom G;
    if (rtw_adapt_geom_of(&p, &G) != 0 || G.local_tiles != tiles || tiles < 1) return 2;
    const size_t floats = (size_t)3 * (size_t)tiles * (size_t)(G.tile_w * G.tile_h);
    float* sums = (float*)malloc(floats * sizeof(float));
    float* squares = (float*)malloc(floats * sizeof(float));
    uint32_t* stop = (uint32_t*)malloc((size_t)tiles * sizeof(uint32_t));
    if (!sums || !squares || !stop) return 2;
    if (fread(sums, 4, floats, f) != floats || fread(squares, 4, floats, f) != floats ||
        fread(stop, 4, (size_t)tiles, f) != (size_t)tiles)
        return 2;
    fclose(f);
    const int rc = rtw_adapt_tiles(sums, squares, &p, u[0], target, u[1], stop);
    printf("rc %d tiles %d\n", rc, (int)tiles);
    for (int32_t t = 0; t < tiles; ++t) printf("%u\n", (unsigned)stop[t]);
    free(sums);
    free(squares);
    free(stop);
    return 0;
}

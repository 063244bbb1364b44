/* The five samplers a path draws from (include/rtw_scalar.h), one chain per start state, written as raw records
 * for tests/test_path_host.py to compare with oracle/pyref.Xoro's: value and end state.
 *
 *   draws_check N  ->  N records of { u64 start[2]; f32 gen, range_a, range_b; u32 coin; f32 sphere[3], ball[3];
 *                                      u64 end[2]; }  on stdout
 *
 * Start state i is (mix64(2 i + 1), mix64(2 i + 2)); the chain is gen_f32, gen_range_f32(213, 343),
 * gen_range_f32(-0.375, 0.0625), gen_bool(0.5), UnitSphere, UnitBall. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/rtw_scalar.h"

typedef struct Record {
    uint64_t start[2];
    float gen, range_a, range_b;
    uint32_t coin;
    float sphere[3], ball[3];
    uint64_t end[2];
} Record;

int main(int argc, char** argv) {
    const long n = argc > 1 ? atol(argv[1]) : 1000;
    for (long i = 0; i < n; ++i) {
        Record r;
        rtw_xoro x;
        x.s0 = rtw_mix64(2u * (uint64_t)i + 1u);
        x.s1 = rtw_mix64(2u * (uint64_t)i + 2u);
        r.start[0] = x.s0;
        r.start[1] = x.s1;
        r.gen = rtw_gen_f32(&x);
        r.range_a = rtw_gen_range_f32(213.0f, 343.0f, &x);
        r.range_b = rtw_gen_range_f32(-0.375f, 0.0625f, &x);
        r.coin = (uint32_t)rtw_gen_bool_half(&x);
        rtw_unit_sphere(&x, r.sphere);
        rtw_unit_ball(&x, r.ball);
        r.end[0] = x.s0;
        r.end[1] = x.s1;
        if (fwrite(&r, sizeof(r), 1, stdout) != 1) return 1;
    }
    return 0;
}

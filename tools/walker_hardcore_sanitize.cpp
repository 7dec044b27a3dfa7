// walker_hardcore_sanitize.cpp -- a stand-alone program over csrc/ses_walker_hardcore_env.h for the host's sanitizers: terrains for
// many keys, random actions on each, every terrain access of the world (collision, time of impact, lidar) and of the generator
// under AddressSanitizer and UBSan.  The new risk of the hardcore env is an index outside a terrain row; this is where it shows.
//
//   g++ -O1 -g -mfma -ffp-contract=off -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I simple-es_amd/csrc -I oracle tools/walker_hardcore_sanitize.cpp -o /tmp/bwh_sanitize -lm && /tmp/bwh_sanitize [keys] [steps]
//
// Each terrain row sits in its own heap block of exactly BWH_ROW floats, so a read or write one byte outside it is reported.
// (Out-of-range float -> int conversions are not: the world's index_of() on a far-away x is as BipedalWalker-v3's.)
#include <stdio.h>
#include <stdlib.h>

#include "../tests/walker_hardcore_host.cpp"

static uint32_t rng_state = 0x12345u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float unit() { return (float)(rng() & 0xFFFF) / 65535.0f; }

int main(int argc, char **argv)
{
    const int keys = argc > 1 ? atoi(argv[1]) : 3000, steps = argc > 2 ? atoi(argv[2]) : 300;
    long long total = 0, on_obstacle = 0, fell = 0, kinds[4] = {0, 0, 0, 0}, max_edges = 0;
    for (int key = 0; key < keys; ++key) {
        float *row = (float *)malloc(sizeof(float) * BWH_ROW);
        uint8_t *kind = (uint8_t *)malloc(BWH_COLS);
        const uint32_t k0 = 0x9E3779B9u * (uint32_t)(key + 1), k1 = (uint32_t)key;
        hardcore_terrain_generate(k0, k1, row, kind);
        for (int c = 0; c < BWH_COLS; ++c) kinds[kind[c]] += 1;
        const HardcoreTerrain terr{row};
        if (terr.n_edges() > max_edges) max_edges = terr.n_edges();
        // every edge, every column's index, a few rays across the whole row
        for (int k = 0; k < terr.n_edges(); ++k) {
            float x1, y1, x2, y2;
            terr.edge(k, x1, y1, x2, y2);
            if (x1 == x2 && y1 == y2) { printf("zero-length edge %d of key %d\n", k, key); return 1; }
        }
        for (float x = -3.0f; x < 100.0f; x += 0.11f) {
            const int i = terr.index_of(x);
            if (i < -1 || i > terr.n_edges()) { printf("index_of(%g) = %d\n", x, i); return 1; }
        }
        (void)walker_raycast(terr, -5.0f, 8.0f, 100.0f, 1.0f);
        // the env: reset, then random actions; now and then the walker is moved further along the row so that every part of it,
        // both ends included, gets a body on it
        WalkerHardcoreEnv *e = (WalkerHardcoreEnv *)malloc(sizeof(WalkerHardcoreEnv));
        memset(e, 0, sizeof *e);
        const float u4[4] = {unit(), 0.0f, 0.0f, 0.0f};
        walker_reset(*e, terr, u4);
        const int mode = key % 3;                       // 0: hold one action, 1: a new action every step, 2: every 10 steps
        float a[4] = {2.0f * unit() - 1.0f, 2.0f * unit() - 1.0f, 2.0f * unit() - 1.0f, 2.0f * unit() - 1.0f};
        if (key % 5 == 0) shift_bodies(*e, unit() * 90.0f - 6.0f, unit() * 1.0f);
        for (int t = 0; t < steps; ++t) {
            if (mode == 1 || (mode == 2 && t % 10 == 0))
                for (int j = 0; j < 4; ++j) a[j] = 2.4f * unit() - 1.2f;
            bool done;
            (void)walker_step(*e, terr, a, done);
            total += 1;
            for (int b = 0; b < 4; ++b)
                for (int s = 0; s < WalkerHardcoreDef::NSLOT; ++s) {
                    const Manifold &m = e->w.mf[b][s];
                    if (m.count > 0 && m.edge >= 0) {
                        const int c = terr.bytes()[BW_TERRAIN_LENGTH + m.edge];
                        on_obstacle += (m.edge != c + terr.bytes()[c]) || kind[c] != BWH_KIND_GROUND;
                    }
                }
            if (done) { fell += 1; break; }
        }
        free(e);
        free(kind);
        free(row);
    }
    printf("%d keys, %lld steps, %lld episodes ended, %lld manifold-steps on obstacle edges, columns by kind %lld %lld %lld %lld, most edges %lld\n",
           keys, total, fell, on_obstacle, kinds[0], kinds[1], kinds[2], kinds[3], max_edges);
    return 0;
}

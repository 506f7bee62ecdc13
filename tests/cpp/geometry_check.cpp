// Host-side check of the tile geometry (tamcmc_dev.h): tile counts keep tiles * TM_TILE_MAXU > units, and the
// equal-cost boundaries of tm_tile_bound -- the same function the setup kernel runs -- cover [0, units) in order with
// tiles of at most TM_TILE_MAXU units, for adversarial and random unit costs.  Also the default block of a posterior
// summary (tms_default_block, tamcmc_summary_walk.h) at every edge of its rule: 64 up to 2^17 bins, 63 one bin later, 2 / 1
// either side of 2^22, still 1 past a row of 64 MiB, and B Nx 8 <= 64 MiB wherever B > 1.  Built and run by
// tests/test_capi_host.py.
#include "tamcmc_dev.h"
#include "tamcmc_summary_walk.h"
#include <cstdio>
#include <vector>

static unsigned long long rng = 88172645463325252ull;
static unsigned next_u32() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (unsigned)(rng >> 32); }

int main() {
    long checked = 0;
    // every unit count up to 700, then steps of 97, then TM_EQ_MAXU - 1 and TM_EQ_MAXU themselves (one unit of slack, none)
    for (int units = 1; units <= TM_EQ_MAXU; units = units < 700 ? units + 1 : (units < TM_EQ_MAXU - 1 && units + 97 > TM_EQ_MAXU - 1) ? TM_EQ_MAXU - 1 : (units == TM_EQ_MAXU - 1) ? TM_EQ_MAXU : units + 97) {
        for (int grad = 0; grad < 2; grad++) {
            const int T = tm_tiles(units, grad);
            if (T < 1 || (long long)T * TM_TILE_MAXU < units) { printf("bad tile count: units %d -> %d\n", units, T); return 1; }
            // the balancer's predicate is the one this check skips by: slack, more than one tile, ranks in LDS
            if (tm_setup_balances(units, T, 1, TM_TILE_MAXU) != ((T > 1 && T <= TM_ORDER_MAX && (long long)T * TM_TILE_MAXU > units) ? 1 : 0) ||
                tm_setup_balances(units, T, 0, TM_TILE_MAXU) != 0 || tm_setup_balances(units, T, 1, TM_TILE_MAXU_L) != 0) {
                printf("bad balancer predicate: units %d T %d\n", units, T); return 1;
            }
            if (T == 1 || (long long)T * TM_TILE_MAXU <= units) continue;      // the balancer needs slack; such grids get equal-length tiles
            for (int pattern = 0; pattern < 6; pattern++) {
                std::vector<int> cost(units), pre(units);
                for (int u = 0; u < units; u++) {
                    switch (pattern) {
                    case 0: cost[u] = 60; break;                                            // flat
                    case 1: cost[u] = 60 + ((u * 7 < units) ? 12800 : 0); break;            // a dense head, a cheap tail
                    case 2: cost[u] = 60 + ((u * 7 > units * 6) ? 12800 : 0); break;        // a cheap head, a dense tail
                    case 3: cost[u] = 60 + (int)(next_u32() % 3000); break;                 // random
                    case 4: cost[u] = 110 + ((u % 23) < 3 ? 9000 : 0); break;               // spikes
                    default: cost[u] = 1 + (int)(next_u32() % 2) * 50000; break;            // extreme contrast
                    }
                }
                long long C = 0, cmin = cost[0];
                for (int u = 0; u < units; u++) { C += cost[u]; pre[u] = (int)C; if (cost[u] < cmin) cmin = cost[u]; }
                int prev = 0;
                long long cmax_tile = 0;
                for (int t = 1; t <= T; t++) {
                    const int b = (t == T) ? units : tm_tile_bound(t, T, units, pre.data(), C, cmin);
                    if (b < prev || b - prev > TM_TILE_MAXU || b > units) { printf("bad boundary: units %d T %d pattern %d tile %d [%d, %d)\n", units, T, pattern, t - 1, prev, b); return 1; }
                    const long long ct = (b > 0 ? pre[b - 1] : 0) - (prev > 0 ? pre[prev - 1] : 0);
                    if (ct > cmax_tile) cmax_tile = ct;
                    prev = b;
                }
                if (prev != units) { printf("bad cover: units %d T %d pattern %d -> %d\n", units, T, pattern, prev); return 1; }
                // balance: with flat costs no tile may exceed the mean by more than one unit's cost
                if (pattern == 0 && cmax_tile > C / T + 2 * 60) { printf("unbalanced flat split: units %d T %d max %lld mean %lld\n", units, T, cmax_tile, C / T); return 1; }
                checked++;
            }
        }
    }
    // the unit bound: TM_EQ_MAXU - 1 units are balanced with one unit of slack, TM_EQ_MAXU have none, one more is too long
    // for the LDS prefix whatever the slack
    if (tm_tiles(TM_EQ_MAXU - 1, 0) * TM_TILE_MAXU - (TM_EQ_MAXU - 1) != 1 || tm_setup_balances(TM_EQ_MAXU - 1, tm_tiles(TM_EQ_MAXU - 1, 0), 1, TM_TILE_MAXU) != 1 ||
        tm_setup_balances(TM_EQ_MAXU, tm_tiles(TM_EQ_MAXU, 0), 1, TM_TILE_MAXU) != 0 || tm_setup_balances(TM_EQ_MAXU, tm_tiles(TM_EQ_MAXU, 0) + 1, 1, TM_TILE_MAXU) != 1 ||
        tm_setup_balances(TM_EQ_MAXU + 1, tm_tiles(TM_EQ_MAXU + 1, 0), 1, TM_TILE_MAXU) != 0 || tm_setup_balances(TM_EQ_MAXU + 1, TM_ORDER_MAX, 1, TM_TILE_MAXU) != 0) {
        printf("bad balancer predicate at TM_EQ_MAXU\n"); return 1;
    }
    // the default block: B = min(64, 64 MiB / (8 Nx)), at least 1
    {
        const long long MiB64 = (long long)64 << 20;
        const struct { long long nx; int B; } edge[] = {
            {1, 64}, {2, 64}, {100000, 64}, {131072, 64}, {131073, 63}, {133152, 63}, {133153, 62}, {2796202, 3}, {2796203, 2},
            {4194304, 2}, {4194305, 1}, {8388608, 1}, {8388609, 1}, {(long long)1 << 31, 1}, {((long long)1 << 31) + 1, 1}};
        for (const auto &e : edge)
            if (tms_default_block(e.nx) != e.B) { printf("bad default block: Nx %lld -> %d, not %d\n", e.nx, tms_default_block(e.nx), e.B); return 1; }
        int prev = 64;
        for (long long nx = 1; nx <= 9000000; nx += (nx < 140000 || (nx > 4190000 && nx < 4200000) || (nx > 8380000 && nx < 8390000)) ? 1 : 997) {
            const int B = tms_default_block(nx);
            // within 64 MiB unless it is the one sample that every block has; the largest such B; never growing with Nx
            if (B < 1 || B > 64 || B > prev || (B > 1 && B * nx * 8 > MiB64) || (B < 64 && (B + 1) * nx * 8 <= MiB64)) {
                printf("bad default block: Nx %lld -> %d\n", nx, B); return 1;
            }
            prev = B;
            checked++;
        }
    }
    printf("ok %ld geometries\n", checked);
    return 0;
}

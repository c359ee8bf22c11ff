/*
 * price_chain_many.c -- a plain-C host of libsvmc.so: prices one two-expiry chain for three LogSV parameter sets, each on its
 * own seed, with ONE svmc_logsv_chain_price_many call (one stepping launch for all jobs), then the same three jobs under
 * Heston (Euler) with svmc_heston_chain_price_many, and prints the results as JSON.
 *
 *   gcc -O2 -Iinclude examples/price_chain_many.c -o price_chain_many -Lstochvolmodels_amd -lsvmc \
 *       -Wl,-rpath,$PWD/stochvolmodels_amd -lm
 *   ./price_chain_many [n_path] [seed]
 *
 * Job j's numbers are those of a single svmc_logsv_chain_price / svmc_heston_chain_price call with job j's parameters and
 * seed + j, and those of stochvolmodels_amd.logsv_mc_chain_pricer_many on the same jobs: tests/test_gpu_mc_many.py.
 */
#include <stdio.h>
#include <stdlib.h>

#include "svmc.h"

#define CHECK(call)                                                                  \
    do {                                                                             \
        int rc_ = (call);                                                            \
        if (rc_ != SVMC_OK) {                                                        \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, svmc_last_error()); \
            return 1;                                                                \
        }                                                                            \
    } while (0)

#define N_JOBS 3
#define N_EXP 2
#define N_K 6

static void print_array(const char *name, const double *a, size_t n, int last)
{
    printf("\"%s\": [", name);
    for (size_t i = 0; i < n; ++i) printf("%s%.17g", i ? ", " : "", a[i]);
    printf("]%s", last ? "" : ", ");
}

int main(int argc, char **argv)
{
    const size_t n_path = (argc > 1) ? (size_t)strtoull(argv[1], NULL, 10) : 65536;
    const uint64_t seed = (argc > 2) ? strtoull(argv[2], NULL, 10) : 20240601ull;

    CHECK(svmc_set_device(0));

    /* chain: ttms 0.1 and 0.25; strikes 0.8, 1.0, 1.2 x forward; P, C, C then IP, IC, C */
    const double ttms[N_EXP] = {0.1, 0.25}, forwards[N_EXP] = {1.0, 1.01}, discfactors[N_EXP] = {0.99, 0.98};
    const double strikes[N_K] = {0.8, 1.0, 1.2, 0.8 * 1.01, 1.0 * 1.01, 1.2 * 1.01};
    const int8_t types[N_K] = {SVMC_PUT, SVMC_CALL, SVMC_CALL, SVMC_INV_PUT, SVMC_INV_CALL, SVMC_CALL};
    const size_t offsets[N_EXP + 1] = {0, 3, 6};

    /* per job: v0 theta kappa1 kappa2 beta volvol, then one vol-backbone eta per expiry (LOGSV_BTC_PARAMS and two variants) */
    const double logsv_params[N_JOBS][6 + N_EXP] = {{0.8376, 1.0413, 3.1844, 3.058, 0.1514, 1.8458, 1.0, 1.0},
                                                     {0.6, 0.7, 2.0, 2.5, -0.3, 1.2, 1.0, 1.0},
                                                     {0.8376, 1.0413, 3.1844, 3.058, 0.1514, 1.8458, 0.9, 1.1}};
    /* per job: v0 theta kappa rho volvol */
    const double heston_params[N_JOBS][5] = {{0.04, 0.04, 4.0, -0.5, 0.4}, {0.09, 0.06, 2.0, -0.7, 0.6}, {0.8, 1.0, 2.0, 0.0, 2.0}};
    uint64_t seeds[N_JOBS];
    uint32_t call_ids[N_JOBS];
    for (int j = 0; j < N_JOBS; ++j) {
        seeds[j] = seed + (uint64_t)j;
        call_ids[j] = 0;    /* a seeded call is call 0 of its stream */
    }
    double prices[N_JOBS * N_K], stderrs[N_JOBS * N_K];

    /* a session sized for the chain, as for a single call: the many-job driver grows its per-job buffers itself */
    svmc_session_t session;
    CHECK(svmc_session_create(&session, n_path, N_EXP, N_K));

    printf("{\"svmc_version\": %d, \"n_path\": %zu, \"seed\": %llu, ", svmc_version(), n_path, (unsigned long long)seed);
    CHECK(svmc_logsv_chain_price_many(session, ttms, forwards, discfactors, N_EXP, strikes, types, offsets, N_JOBS,
                                      &logsv_params[0][0], seeds, call_ids, /*spot measure*/ 1, /*steps per year*/ 120,
                                      SVMC_LOG_RETURN, prices, stderrs));
    print_array("logsv_prices", prices, N_JOBS * N_K, 0);
    print_array("logsv_stderrs", stderrs, N_JOBS * N_K, 0);

    CHECK(svmc_heston_chain_price_many(session, ttms, forwards, discfactors, N_EXP, strikes, types, offsets, N_JOBS,
                                       &heston_params[0][0], seeds, call_ids, SVMC_HESTON_EULER_FLOOR, 360, SVMC_LOG_RETURN,
                                       prices, stderrs));
    print_array("heston_prices", prices, N_JOBS * N_K, 0);
    print_array("heston_stderrs", stderrs, N_JOBS * N_K, 1);
    printf("}\n");

    CHECK(svmc_session_destroy(session));
    return 0;
}

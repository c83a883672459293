/* values_plan_check.c -- the plan builder and the host apply of the bulk value update (spx_hip_mat_values_plan,
 * spx_hip_mat_set_values_host) under a sanitizer, from a program of its own: a general matrix, a symmetric one
 * and a pattern that is not the tuned one, on host-only tunes.  Build and run (no GPU needed):
 *
 *   tools/build_asan.sh
 *   gcc -std=gnu11 -g -fsanitize=address,undefined -Iinclude tools/values_plan_check.c \
 *       -Lsparsex_amd/lib/variants -lsparsex_asan -Wl,-rpath,$PWD/sparsex_amd/lib/variants -lm -o build/values_plan_check
 *   build/values_plan_check
 *
 * (leak detection stays on: the failure path of the plan and the drop must free what they built)
 *
 * Exit status 0 and "values plan check: ok" when every value reads back and the bad pattern is refused. */
#include <sparsex/sparsex.h>
#include <sparsex_hip.h>

#include <stdio.h>
#include <stdlib.h>

#define N 1500

static int fails = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "line %d: %s\n", __LINE__, #cond);              \
            ++fails;                                                        \
        }                                                                   \
    } while (0)

/* a banded pattern with a few far couplings, symmetric, with a full diagonal; rows sorted by column */
static int build(spx_index_t *rowptr, spx_index_t *colind)
{
    static const int off[] = {-701, -40, -3, -2, -1, 0, 1, 2, 3, 40, 701};
    int nnz = 0;
    for (int r = 0; r < N; ++r) {
        rowptr[r] = nnz;
        for (size_t k = 0; k < sizeof(off) / sizeof(off[0]); ++k) {
            const int c = r + off[k];
            /* (the far couplings only on every third row pair: irregular enough to leave leftovers) */
            if (c < 0 || c >= N) continue;
            if ((off[k] == 701 && r % 3) || (off[k] == -701 && c % 3)) continue;
            colind[nnz++] = c;
        }
    }
    rowptr[N] = nnz;
    return nnz;
}

static double value_at(int r, int c, int seed)
{
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    return 1.0 + ((lo * 7919 + hi * 104729 + seed * 31) % 1000) / 1000.0 + (r == c ? 20.0 : 0.0);
}

static void check(int symmetric, const spx_index_t *rowptr, const spx_index_t *colind, int nnz)
{
    double *v0 = malloc(sizeof(double) * (size_t) nnz), *v1 = malloc(sizeof(double) * (size_t) nnz);
    for (int r = 0; r < N; ++r)
        for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) {
            v0[k] = value_at(r, colind[k], 1);
            v1[k] = value_at(r, colind[k], 2);
        }
    spx_hip_options_reset();
    spx_option_set("spx.rt.host_only", "true");
    spx_option_set("spx.preproc.sampling", "none");
    spx_option_set("spx.matrix.symmetric", symmetric ? "true" : "false");
    spx_input_t *in = spx_input_load_csr(rowptr, colind, v0, N, N, SPX_INDEX_ZERO_BASED);
    spx_matrix_t *A = spx_mat_tune(in);
    EXPECT(A != SPX_INVALID_MAT);
    EXPECT(spx_hip_mat_set_values_host(A, v1) == SPX_FAILURE);            /* no plan yet */
    EXPECT(spx_hip_mat_values_plan(A, rowptr, colind, SPX_INDEX_ZERO_BASED) == SPX_SUCCESS);
    spx_hip_values_plan_t plan;
    EXPECT(spx_hip_mat_values_plan_get(A, &plan) == SPX_SUCCESS);
    EXPECT(plan.plan_bytes == 0 && plan.n_dest >= plan.n_sources && plan.n_sources > 0);
    uint64_t with_source = 0;
    for (size_t i = 0; i < plan.n_values; ++i) with_source += plan.src_values[i] != 0xffffffffu;
    for (size_t i = 0; i < plan.n_diag; ++i) with_source += plan.src_diag[i] != 0xffffffffu;
    for (size_t i = 0; i < plan.n_mirror; ++i) with_source += plan.src_mirror[i] != 0xffffffffu;
    EXPECT(with_source == plan.n_dest);
    EXPECT(spx_hip_mat_set_values_host(A, v1) == SPX_SUCCESS);
    for (int r = 0; r < N; ++r)
        for (int k = rowptr[r]; k < rowptr[r + 1]; ++k) {
            double got = 0.0;
            EXPECT(spx_mat_get_entry(A, r, colind[k], &got, SPX_INDEX_ZERO_BASED) == SPX_SUCCESS && got == v1[k]);
        }
    /* a pattern that is not the tuned one: one column moved; refused, no plan left, the values untouched */
    spx_index_t *moved = malloc(sizeof(spx_index_t) * (size_t) nnz);
    for (int k = 0; k < nnz; ++k) moved[k] = colind[k];
    moved[rowptr[N / 2] + 1] = colind[rowptr[N / 2] + 1] == N / 2 - 39 ? N / 2 - 41 : N / 2 - 39;
    EXPECT(spx_hip_mat_values_plan(A, rowptr, moved, SPX_INDEX_ZERO_BASED) == SPX_FAILURE);
    EXPECT(spx_hip_mat_values_plan_get(A, &plan) == SPX_FAILURE);
    EXPECT(spx_hip_mat_set_values_host(A, v0) == SPX_FAILURE);
    double got = 0.0;
    EXPECT(spx_mat_get_entry(A, N / 2, N / 2, &got, SPX_INDEX_ZERO_BASED) == SPX_SUCCESS && got == value_at(N / 2, N / 2, 2));
    /* ... and back to the values of the tune through a new plan, then without one */
    EXPECT(spx_hip_mat_values_plan(A, rowptr, colind, SPX_INDEX_ZERO_BASED) == SPX_SUCCESS);
    EXPECT(spx_hip_mat_set_values_host(A, v0) == SPX_SUCCESS);
    EXPECT(spx_mat_get_entry(A, N - 1, N - 2, &got, SPX_INDEX_ZERO_BASED) == SPX_SUCCESS && got == value_at(N - 1, N - 2, 1));
    EXPECT(spx_hip_mat_values_plan_drop(A) == SPX_SUCCESS);
    EXPECT(spx_hip_mat_set_values_host(A, v1) == SPX_FAILURE);
    spx_mat_destroy(A);
    spx_input_destroy(in);
    free(moved);
    free(v0);
    free(v1);
}

int main(void)
{
    spx_init();
    spx_log_disable_all();
    spx_index_t *rowptr = malloc(sizeof(spx_index_t) * (N + 1)), *colind = malloc(sizeof(spx_index_t) * N * 11);
    const int nnz = build(rowptr, colind);
    check(0, rowptr, colind, nnz);
    check(1, rowptr, colind, nnz);
    free(rowptr);
    free(colind);
    printf("values plan check: %s (%d entries, general and symmetric)\n", fails ? "FAILED" : "ok", nnz);
    return fails ? 1 : 0;
}

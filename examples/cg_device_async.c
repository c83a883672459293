/*
 * cg_device_async.c -- the loop of cg_device.c without a host round trip in it:
 * the scalars of the iteration (r.r, p.Ap, beta) live in a three-element device
 * vector, the dot product writes there (spx_hip_vec_mul_dev), the update of x
 * and r with the new r.r and beta is one fused call (spx_hip_vec_cg_update), and
 * p = r + beta p reads beta from the device (spx_hip_vec_scale_add_ratio).  Every
 * call of an iteration only enqueues, so the stream never drains (and the loop
 * body could be captured into a hipGraph); r.r is downloaded every tenth
 * iteration to test convergence.  Plain C against the C ABI of libsparsex.so:
 *
 *   gcc examples/cg_device_async.c -Iinclude -Lsparsex_amd/lib -lsparsex \
 *       -Wl,-rpath,$PWD/sparsex_amd/lib -lm -o cg_device_async && ./cg_device_async 300
 */
#include <sparsex/sparsex.h>
#include <sparsex_hip.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv)
{
    const int g = argc > 1 ? atoi(argv[1]) : 200;      /* g x g grid */
    const int n = g * g;
    spx_index_t *rowptr = malloc((n + 1) * sizeof(*rowptr));
    spx_index_t *colind = malloc((size_t) 5 * n * sizeof(*colind));
    spx_value_t *values = malloc((size_t) 5 * n * sizeof(*values));
    int nnz = 0;
    for (int i = 0; i < g; i++)
        for (int j = 0; j < g; j++) {
            const int r = i * g + j;
            rowptr[r] = nnz;
            if (i > 0) { colind[nnz] = r - g; values[nnz++] = -1.0; }
            if (j > 0) { colind[nnz] = r - 1; values[nnz++] = -1.0; }
            colind[nnz] = r; values[nnz++] = 4.0;
            if (j < g - 1) { colind[nnz] = r + 1; values[nnz++] = -1.0; }
            if (i < g - 1) { colind[nnz] = r + g; values[nnz++] = -1.0; }
        }
    rowptr[n] = nnz;

    spx_init();
    spx_option_set("spx.matrix.symmetric", "true");     /* stored once, used twice */
    spx_input_t *in = spx_input_load_csr(rowptr, colind, values, n, n, SPX_INDEX_ZERO_BASED);
    spx_matrix_t *A = spx_mat_tune(in);
    if (!A) return 1;

    /* b = A * ones, so the solution is the vector of ones */
    spx_hip_vec_t *x = spx_hip_vec_create(n), *b = spx_hip_vec_create(n);
    spx_hip_vec_t *r = spx_hip_vec_create(n), *p = spx_hip_vec_create(n), *ap = spx_hip_vec_create(n);
    spx_hip_vec_init(p, 1.0, NULL);
    spx_hip_matvec_kernel_vec(1.0, A, p, 0.0, b, NULL);
    spx_hip_vec_copy(b, r, NULL);                        /* x0 = 0  =>  r0 = b */
    spx_hip_vec_copy(r, p, NULL);
    /* device scalars: sc[0] = r.r, sc[1] = p.Ap, sc[2] = beta */
    spx_hip_vec_t *sc = spx_hip_vec_create(3);
    spx_value_t *rr_dev = spx_hip_vec_data(sc), *pap_dev = rr_dev + 1, *beta_dev = rr_dev + 2;
    spx_value_t sch[3];
    spx_vector_t *scv = spx_vec_create_from_buff(sch, NULL, 3, NULL, SPX_VEC_AS_IS);
    double rr, rr0;
    spx_hip_vec_mul_dev(r, r, rr_dev, NULL);
    spx_hip_vec_download(sc, scv, NULL);
    rr = rr0 = sch[0];
    int it = 0;
    while (rr > 1e-20 * rr0 && it < 10 * g) {
        for (int k = 0; k < 10; k++) {                               /* nothing here waits for the GPU */
            spx_hip_matvec_kernel_vec(1.0, A, p, 0.0, ap, NULL);                  /* ap = A p       */
            spx_hip_vec_mul_dev(p, ap, pap_dev, NULL);                            /* pap = p . ap   */
            spx_hip_vec_cg_update(x, p, r, ap, rr_dev, pap_dev, beta_dev, NULL);  /* x, r, rr, beta */
            spx_hip_vec_scale_add_ratio(r, p, p, 1.0, beta_dev, NULL, NULL);      /* p = r + beta p */
        }
        it += 10;
        spx_hip_vec_download(sc, scv, NULL);
        rr = sch[0];
    }

    spx_value_t *xh = malloc(n * sizeof(*xh));
    spx_vector_t *xv = spx_vec_create_from_buff(xh, NULL, n, NULL, SPX_VEC_AS_IS);
    spx_hip_vec_download(x, xv, NULL);
    double err = 0.0;
    for (int i = 0; i < n; i++) err = fmax(err, fabs(xh[i] - 1.0));
    printf("n = %d, nnz = %d: %d CG iterations, |r|/|b| = %.3e, max |x - 1| = %.3e\n", n, nnz, it,
           sqrt(rr / rr0), err);

    spx_vec_destroy(xv);
    spx_vec_destroy(scv);
    spx_hip_vec_destroy(sc);
    spx_hip_vec_destroy(x); spx_hip_vec_destroy(b); spx_hip_vec_destroy(r);
    spx_hip_vec_destroy(p); spx_hip_vec_destroy(ap);
    spx_mat_destroy(A);
    spx_input_destroy(in);
    free(rowptr); free(colind); free(values); free(xh);
    return err < 1e-6 ? 0 : 2;
}

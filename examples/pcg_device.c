/*
 * pcg_device.c -- Jacobi-preconditioned CG that never leaves the GPU: the loop of
 * cg_device_async.c on a badly scaled SPD system, D A D with A the 5-point
 * Laplacian and d_i = 10^u_i, u_i uniform in (-1, 1).  Plain CG crawls on it;
 * with the inverse of the diagonal as preconditioner it converges like CG on A.
 *
 * The preconditioner comes from the tuned matrix: spx_hip_mat_diag_plan (once),
 * spx_hip_mat_get_diag_vec and spx_hip_vec_reciprocal.  An iteration is four
 * calls that only enqueue -- the product, p.Ap (spx_hip_vec_mul_dev), the fused
 * update of x, r, r.z, r.r and beta (spx_hip_vec_pcg_update) and the new search
 * direction (spx_hip_vec_pcg_direction) -- with no z vector and no host round
 * trip; r.z is downloaded every tenth iteration to test convergence.  Plain C
 * against the C ABI of libsparsex.so:
 *
 *   gcc examples/pcg_device.c -Iinclude -Lsparsex_amd/lib -lsparsex \
 *       -Wl,-rpath,$PWD/sparsex_amd/lib -lm -o pcg_device && ./pcg_device 60
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
    double *d = malloc(n * sizeof(*d));
    unsigned long long lcg = 11;
    for (int i = 0; i < n; i++) {
        lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
        d[i] = pow(10.0, 2.0 * (double) (lcg >> 11) / 9007199254740992.0 - 1.0);
    }
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
    for (int r = 0; r < n; r++)                          /* D A D */
        for (int k = rowptr[r]; k < rowptr[r + 1]; k++) values[k] *= d[r] * d[colind[k]];

    spx_init();
    spx_input_t *in = spx_input_load_csr(rowptr, colind, values, n, n, SPX_INDEX_ZERO_BASED);
    spx_matrix_t *A = spx_mat_tune(in);
    if (!A) return 1;

    /* b = A * ones, so the solution is the vector of ones */
    spx_hip_vec_t *x = spx_hip_vec_create(n), *b = spx_hip_vec_create(n), *minv = spx_hip_vec_create(n);
    spx_hip_vec_t *r = spx_hip_vec_create(n), *p = spx_hip_vec_create(n), *ap = spx_hip_vec_create(n);
    spx_hip_vec_init(p, 1.0, NULL);
    spx_hip_matvec_kernel_vec(1.0, A, p, 0.0, b, NULL);
    spx_hip_vec_copy(b, r, NULL);                        /* x0 = 0  =>  r0 = b */
    /* the Jacobi preconditioner: minv = 1 / diag(A), read from the tuned matrix in HBM */
    if (spx_hip_mat_diag_plan(A) != SPX_SUCCESS || spx_hip_mat_get_diag_vec(A, minv, NULL) != SPX_SUCCESS ||
        spx_hip_vec_reciprocal(minv, minv, 1.0, NULL) != SPX_SUCCESS)
        return 1;
    /* device scalars: sc[0] = r.z, sc[1] = p.Ap, sc[2] = beta, sc[3] = r.r (a fresh vector holds zeros) */
    spx_hip_vec_t *sc = spx_hip_vec_create(4);
    spx_value_t *rz_dev = spx_hip_vec_data(sc), *pap_dev = rz_dev + 1, *beta_dev = rz_dev + 2, *rr_dev = rz_dev + 3;
    spx_value_t sch[4];
    spx_vector_t *scv = spx_vec_create_from_buff(sch, NULL, 4, NULL, SPX_VEC_AS_IS);
    double rz, rz0;
    /* start-up: with r.z = p.Ap = 0 the update leaves x and r alone and writes r.z and r.r; then p0 = minv .* r */
    spx_hip_vec_pcg_update(x, p, r, ap, minv, rz_dev, pap_dev, beta_dev, rr_dev, NULL);
    spx_hip_vec_pcg_direction(p, r, minv, NULL, NULL);
    spx_hip_vec_download(sc, scv, NULL);
    rz = rz0 = sch[0];
    int it = 0;
    while (rz > 1e-24 * rz0 && it < 10 * g) {
        for (int k = 0; k < 10; k++) {                               /* nothing here waits for the GPU */
            spx_hip_matvec_kernel_vec(1.0, A, p, 0.0, ap, NULL);                                  /* ap = A p             */
            spx_hip_vec_mul_dev(p, ap, pap_dev, NULL);                                            /* pap = p . ap         */
            spx_hip_vec_pcg_update(x, p, r, ap, minv, rz_dev, pap_dev, beta_dev, rr_dev, NULL);   /* x, r, rz, rr, beta   */
            spx_hip_vec_pcg_direction(p, r, minv, beta_dev, NULL);                                /* p = minv.*r + beta p */
        }
        it += 10;
        spx_hip_vec_download(sc, scv, NULL);
        rz = sch[0];
    }

    spx_value_t *xh = malloc(n * sizeof(*xh));
    spx_vector_t *xv = spx_vec_create_from_buff(xh, NULL, n, NULL, SPX_VEC_AS_IS);
    spx_hip_vec_download(x, xv, NULL);
    double err = 0.0;
    for (int i = 0; i < n; i++) err = fmax(err, fabs(xh[i] - 1.0));
    printf("n = %d, nnz = %d: %d PCG iterations, r.z / r0.z0 = %.3e, max |x - 1| = %.3e\n", n, nnz, it, rz / rz0, err);

    spx_vec_destroy(xv);
    spx_vec_destroy(scv);
    spx_hip_vec_destroy(sc);
    spx_hip_vec_destroy(x); spx_hip_vec_destroy(b); spx_hip_vec_destroy(r);
    spx_hip_vec_destroy(p); spx_hip_vec_destroy(ap); spx_hip_vec_destroy(minv);
    spx_mat_destroy(A);
    spx_input_destroy(in);
    free(rowptr); free(colind); free(values); free(xh); free(d);
    return err < 1e-6 ? 0 : 2;
}

/* N-API shim: the thin Node.js <-> C-ABI binding of include/nd4hip.h (north_star: "the Node.js host
 * keeps the nd.la API surface and calls into a thin N-API C-ABI addon").
 *
 * Plain C, built without node-gyp:  gcc -shared -fPIC -I/usr/include/node napi_shim.c -ldl
 * libnd4hip.so is dlopen'ed from the directory above this addon, so the addon itself has no HIP
 * link-time dependency. Every array operand of a compute export is EITHER
 *   - a TypedArray (host memory, exactly what NDArray.data is in the reference, src/nd_array.js:135-147):
 *     the HOST-pointer entry points run H2D -> kernels -> D2H synchronously, the blocking semantics of
 *     the reference's JS functions; OR
 *   - a device view {b: <buffer from dev_alloc>, o: <element offset>} (device-resident
 *     NDArray): the `_dev` entry points run on the handle's stream and nothing crosses PCIe.
 * All operands of one call must live on the same side. Errors become JS exceptions carrying
 * nd4hip_last_error(). There is no CPU fallback here.
 */
#define _GNU_SOURCE
#define NAPI_VERSION 6
#include <node_api.h>
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "nd4hip.h"

static void* g_lib = NULL;
static nd4hip_handle* g_handle = NULL;

typedef int (*gemm_fn)(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, double*);
typedef int (*getrf_fn)(nd4hip_handle*, int64_t, int64_t, const double*, double*, int32_t*);
typedef int (*geqrf_fn)(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*);
typedef int (*gesvdj_fn)(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*, double*, int*, double*);
typedef int (*qrls_fn)(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, const double*, int64_t, double*);
typedef int (*svdls_fn)(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, const double*, int64_t,
                        const double*, int64_t, double*);
typedef int (*getrs_fn)(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, int64_t, const int32_t*, int64_t, const double*, int64_t, double*);
typedef int (*trsm_fn)(nd4hip_handle*, int, int, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, double*);

static int  (*p_device_count)(void);
static int  (*p_create_multi)(nd4hip_handle**, const int*, int);
static int  (*p_device_list)(nd4hip_handle*, int*, int);
static int  (*p_create)(nd4hip_handle**, int);
static void (*p_destroy)(nd4hip_handle*);
static const char* (*p_last_error)(void);
static const char* (*p_version)(void);
/* [0] = host-pointer entry point, [1] = its _dev twin */
static gemm_fn p_dgemm[2];
static int (*p_zgemm[2])(nd4hip_handle*, int, int, int64_t, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, double*);
static getrf_fn p_dgetrf[2];
static geqrf_fn p_dgeqrf[2];
static geqrf_fn p_dgeqrf_full[2];
static int (*p_dgebrd[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*, double*);
static int (*p_dgehrd[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*);
static int (*p_dgeqrf_qty[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, double*, double*);
static gesvdj_fn p_dgesvdj[2];
static int (*p_dgesdd[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*, double*);
static int (*p_svd_info)(nd4hip_handle*, int*, unsigned long long*, double*);
static qrls_fn p_dqrls[2];
static int (*p_dgeqp3[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*, int32_t*);
static int (*p_dgeqp3_full[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*, int32_t*);
static int (*p_dsrrqr[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double, double, double*, double*, int32_t*, int32_t*);
static int (*p_durv[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*, double*, int32_t*);
static int (*p_durvls[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t,
                          const double*, int64_t, const int32_t*, int64_t, const double*, int64_t, double*);
static int (*p_ddet[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*);
static int (*p_dslogdet[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*, double*);
static int (*p_ddettri[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*);
static int (*p_dslogdettri[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*);
static int (*p_dnrmfro[2])(nd4hip_handle*, int64_t, const double*, double*);
static int (*p_dtreval[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*);
static int (*p_dtrevc[2])(nd4hip_handle*, int64_t, int64_t, const double*, const double*, double*, double*);
static int (*p_dgebal[2])(nd4hip_handle*, int64_t, int64_t, double, const double*, double*, double*);
static int (*p_zgebak[2])(nd4hip_handle*, int64_t, int64_t, const double*, const double*, double*);
static int (*p_dhseqr[2])(nd4hip_handle*, int64_t, int64_t, const double*, const double*, double*, double*, int*);
static int (*p_dgees[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*, int*);
static int (*p_dgeev[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*);
static int (*p_dsyevd[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*);
static int (*p_dsyevj[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*, int32_t*);
static int (*p_dsyevx[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, const double*, double*, double*);
static int (*p_dsyevd_tr[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*);
static int (*p_dsyevx_tr[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, const double*, double*, double*);
static int (*p_zheevd[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*, double*);
static int (*p_zheevx[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, const double*, double*, double*);
static int (*p_zpotrf[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*);
static int (*p_zpotrs[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, int64_t, const double*, double*);
static int (*p_zhegvd[2])(nd4hip_handle*, int64_t, int64_t, const double*, const double*, int64_t, double*, double*);
static int (*p_zhegvx[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, const double*, const double*, int64_t, double*, double*);
static int (*p_dsygvd[2])(nd4hip_handle*, int, int64_t, int64_t, const double*, const double*, int64_t, double*, double*, int32_t*);
static int (*p_dstcnt[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, const double*, const double*, int32_t*);
static int (*p_dstevx[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, const double*, const double*, double*, double*);
static int (*p_dbdsvdx[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, int64_t, const double*, const double*, double*, double*, double*, int32_t*);
static int (*p_dgesvdx[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, int64_t, const double*, double*, double*, double*, int32_t*);
static int (*p_dstevxv[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, const double*, const double*, double*, double*, int32_t*, int64_t*);
static int (*p_dsyevxv[2][2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, const double*, double*, double*, int32_t*, int64_t*);   /* [tridiag][dev] */
static int (*p_dsygvx[2])(nd4hip_handle*, int, int, int64_t, int64_t, int64_t, int64_t, int64_t, const double*, const double*, const double*, int64_t,
                          double*, double*, int32_t*, int64_t*);
static int (*p_dqp3rank[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, int32_t*);
static int (*p_dqp3ls[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t,
                          const int32_t*, int64_t, const double*, int64_t, double*, int32_t*);
static svdls_fn p_dsvdls[2];
static getrs_fn p_dgetrs[2];
static int (*p_dpotrf[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*);
static int (*p_dldltrf[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*);
static int (*p_dldltrs[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, double*);
static int (*p_dsytrf_bk[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*, int32_t*, int);
static int (*p_dsytrs_bk[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, int64_t, const int32_t*, int64_t, const double*, int64_t, double*);
static int (*p_dtranspose[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, double*);
static int (*p_dtri[2])(nd4hip_handle*, int, int64_t, int64_t, int64_t, int64_t, const double*, double*);
static int (*p_ddiag[2])(nd4hip_handle*, int64_t, int64_t, int64_t, int64_t, const double*, double*);
static int (*p_ddiagmat[2])(nd4hip_handle*, int64_t, int64_t, const double*, double*);
static int (*p_dpermute[2])(nd4hip_handle*, int, int, int64_t, int64_t, int64_t, const double*, int64_t, const int32_t*, int64_t, double*);
static int (*p_dpotrs[2])(nd4hip_handle*, int64_t, int64_t, int64_t, const double*, int64_t, const double*, int64_t, double*);
static trsm_fn p_dtrsm[2];
static int (*p_malloc)(nd4hip_handle*, size_t, void**);
static int (*p_free)(nd4hip_handle*, void*);
static int (*p_h2d)(nd4hip_handle*, void*, const void*, size_t);
static int (*p_gather_nd)(nd4hip_handle*, int, int, const int64_t*, const void*, int64_t, int64_t, const int64_t*, void*, int64_t, int64_t,
                         const int64_t*);
static int (*p_zip_nd)(nd4hip_handle*, int, int, const int64_t*, const double*, int64_t, int64_t, const int64_t*, const double*, int64_t, int64_t,
                       const int64_t*, double*, int64_t);
static int (*p_reduce_nd)(nd4hip_handle*, int, int, const int64_t*, const int32_t*, const double*, int64_t, double*, int64_t);
static int (*p_d2h)(nd4hip_handle*, void*, const void*, size_t);
static int (*p_sync)(nd4hip_handle*);
static int (*p_prof_enable)(nd4hip_handle*, int);
static int (*p_prof_last)(nd4hip_handle*, nd4hip_prof*, int);

static char g_load_error[4608] = "";

static int load_library(void) {
  if (g_lib) return 0;
  Dl_info info;
  char path[4096];
  const char* env = getenv("ND4HIP_LIBRARY");
  if (env && *env) {
    snprintf(path, sizeof path, "%s", env);
  } else if (dladdr((void*)&load_library, &info) && info.dli_fname) {
    snprintf(path, sizeof path, "%s", info.dli_fname);
    char* slash = strrchr(path, '/');                   /* .../nd4js_amd/js/nd4hip_napi.node */
    if (slash) *slash = 0;
    slash = strrchr(path, '/');                         /* .../nd4js_amd/js */
    if (slash) *slash = 0;
    strncat(path, "/libnd4hip.so", sizeof path - strlen(path) - 1);
  } else {
    snprintf(path, sizeof path, "libnd4hip.so");
  }
  g_lib = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
  if (!g_lib) { snprintf(g_load_error, sizeof g_load_error, "cannot load %s: %s (no CPU fallback)", path, dlerror()); return -1; }
#define SYM(var, name) do { *(void**)(&var) = dlsym(g_lib, name); \
    if (!var) { snprintf(g_load_error, sizeof g_load_error, "symbol %s missing in %s", name, path); return -1; } } while (0)
  SYM(p_device_count, "nd4hip_device_count");
  SYM(p_create_multi, "nd4hip_create_multi");
  SYM(p_device_list, "nd4hip_device_list");
  SYM(p_create, "nd4hip_create");
  SYM(p_destroy, "nd4hip_destroy");
  SYM(p_last_error, "nd4hip_last_error");
  SYM(p_version, "nd4hip_version");
#define SYM2(var, name) SYM(var[0], name); SYM(var[1], name "_dev")
  SYM2(p_dgemm, "nd4hip_dgemm_batched");
  SYM2(p_zgemm, "nd4hip_zgemm_batched");
  SYM2(p_dgetrf, "nd4hip_dgetrf_batched");
  SYM2(p_dgeqrf, "nd4hip_dgeqrf_q_batched");
  SYM2(p_dgeqrf_full, "nd4hip_dgeqrf_full_batched");
  SYM2(p_dgeqrf_qty, "nd4hip_dgeqrf_qty_batched");
  SYM2(p_dgehrd, "nd4hip_dgehrd_batched");
  SYM2(p_dgebrd, "nd4hip_dgebrd_batched");
  SYM2(p_dgesvdj, "nd4hip_dgesvdj_batched");
  SYM2(p_dgesdd, "nd4hip_dgesdd_batched");
  SYM2(p_dgetrs, "nd4hip_dgetrs_batched");
  SYM2(p_dpotrf, "nd4hip_dpotrf_batched");
  SYM2(p_dpotrs, "nd4hip_dpotrs_batched");
  SYM2(p_dldltrf, "nd4hip_dldltrf_batched");
  SYM2(p_dldltrs, "nd4hip_dldltrs_batched");
  SYM2(p_dsytrf_bk, "nd4hip_dsytrf_bk_batched_ex");
  SYM2(p_dsytrs_bk, "nd4hip_dsytrs_bk_batched");
  SYM2(p_dtranspose, "nd4hip_dtranspose_batched");
  SYM2(p_dtri, "nd4hip_dtri_batched");
  SYM2(p_ddiag, "nd4hip_ddiag_batched");
  SYM2(p_ddiagmat, "nd4hip_ddiagmat_batched");
  SYM2(p_dpermute, "nd4hip_dpermute_batched");
  SYM2(p_dqrls, "nd4hip_dqrls_batched");
  SYM2(p_dgeqp3, "nd4hip_dgeqp3_batched");
  SYM2(p_dgeqp3_full, "nd4hip_dgeqp3_full_batched");
  SYM2(p_ddet, "nd4hip_ddet_batched");
  SYM2(p_dslogdet, "nd4hip_dslogdet_batched");
  SYM2(p_ddettri, "nd4hip_ddettri_batched");
  SYM2(p_dslogdettri, "nd4hip_dslogdettri_batched");
  SYM(p_dnrmfro[0], "nd4hip_dnrmfro"); SYM(p_dnrmfro[1], "nd4hip_dnrmfro_dev");
  SYM2(p_dtreval, "nd4hip_dtreval_batched");
  SYM2(p_dtrevc, "nd4hip_dtrevc_batched");
  SYM2(p_dgebal, "nd4hip_dgebal_batched");
  SYM2(p_zgebak, "nd4hip_zgebak_batched");
  SYM2(p_dhseqr, "nd4hip_dhseqr_batched");
  SYM2(p_dgees, "nd4hip_dgees_batched");
  SYM2(p_dgeev, "nd4hip_dgeev_batched");
  SYM2(p_dsyevd, "nd4hip_dsyevd_batched");
  SYM2(p_dsyevj, "nd4hip_dsyevj_batched");
  SYM(p_dsyevx[0], "nd4hip_dsyevx_batched_host"); SYM(p_dsyevx[1], "nd4hip_dsyevx_batched_dev");   /* this pair's host form ends in _host */
  SYM(p_dsyevd_tr[0], "nd4hip_dsyevd_tr_batched_host"); SYM(p_dsyevd_tr[1], "nd4hip_dsyevd_tr_batched_dev");   /* and so do these two */
  SYM(p_dsyevx_tr[0], "nd4hip_dsyevx_tr_batched_host"); SYM(p_dsyevx_tr[1], "nd4hip_dsyevx_tr_batched_dev");
  SYM(p_zheevd[0], "nd4hip_zheevd_batched_host"); SYM(p_zheevd[1], "nd4hip_zheevd_batched_dev");
  SYM(p_zheevx[0], "nd4hip_zheevx_batched_host"); SYM(p_zheevx[1], "nd4hip_zheevx_batched_dev");
  SYM(p_zpotrf[0], "nd4hip_zpotrf_batched_host"); SYM(p_zpotrf[1], "nd4hip_zpotrf_batched_dev");
  SYM(p_zpotrs[0], "nd4hip_zpotrs_batched_host"); SYM(p_zpotrs[1], "nd4hip_zpotrs_batched_dev");
  SYM(p_zhegvd[0], "nd4hip_zhegvd_batched_host"); SYM(p_zhegvd[1], "nd4hip_zhegvd_batched_dev");
  SYM(p_zhegvx[0], "nd4hip_zhegvx_batched_host"); SYM(p_zhegvx[1], "nd4hip_zhegvx_batched_dev");
  SYM2(p_dsygvd, "nd4hip_dsygvd_batched");
  SYM(p_dstcnt[0], "nd4hip_dstcnt_batched_host"); SYM(p_dstcnt[1], "nd4hip_dstcnt_batched_dev");
  SYM(p_dstevx[0], "nd4hip_dstevx_batched_host"); SYM(p_dstevx[1], "nd4hip_dstevx_batched_dev");
  SYM(p_dbdsvdx[0], "nd4hip_dbdsvdx_batched_host"); SYM(p_dbdsvdx[1], "nd4hip_dbdsvdx_batched_dev");
  SYM(p_dgesvdx[0], "nd4hip_dgesvdx_batched_host"); SYM(p_dgesvdx[1], "nd4hip_dgesvdx_batched_dev");
  SYM(p_dstevxv[0], "nd4hip_dstevxv_batched_host"); SYM(p_dstevxv[1], "nd4hip_dstevxv_batched_dev");
  SYM(p_dsyevxv[0][0], "nd4hip_dsyevxv_batched_host"); SYM(p_dsyevxv[0][1], "nd4hip_dsyevxv_batched_dev");
  SYM(p_dsyevxv[1][0], "nd4hip_dsyevxv_tr_batched_host"); SYM(p_dsyevxv[1][1], "nd4hip_dsyevxv_tr_batched_dev");
  SYM(p_dsygvx[0], "nd4hip_dsygvx_batched_host"); SYM(p_dsygvx[1], "nd4hip_dsygvx_batched_dev");
  SYM2(p_dqp3rank, "nd4hip_dqp3rank_batched");
  SYM2(p_dsrrqr, "nd4hip_dsrrqr_batched");
  SYM2(p_durv, "nd4hip_durv_batched");
  SYM2(p_durvls, "nd4hip_durvls_batched");
  SYM2(p_dqp3ls, "nd4hip_dqp3ls_batched");
  SYM2(p_dsvdls, "nd4hip_dsvdls_batched");
  SYM2(p_dtrsm, "nd4hip_dtrsm_batched");
#undef SYM2
  SYM(p_gather_nd, "nd4hip_gather_nd_dev");
  SYM(p_zip_nd, "nd4hip_dzip_nd_dev");
  SYM(p_reduce_nd, "nd4hip_dreduce_nd_dev");
  SYM(p_svd_info, "nd4hip_dgesvdj_last_info");
  SYM(p_malloc, "nd4hip_malloc");
  SYM(p_free, "nd4hip_free");
  SYM(p_h2d, "nd4hip_memcpy_h2d");
  SYM(p_d2h, "nd4hip_memcpy_d2h");
  SYM(p_sync, "nd4hip_synchronize");
  SYM(p_prof_enable, "nd4hip_profile_enable");
  SYM(p_prof_last, "nd4hip_profile_last");
#undef SYM
  return 0;
}

#define THROW(env, msg) do { napi_throw_error((env), "ND4HIP", (msg)); return NULL; } while (0)

/* lazily created, idempotent (the reference has no init step: SURVEY.md §3.5) */
static int ensure_handle(napi_env env) {
  if (load_library() != 0) { napi_throw_error(env, "ND4HIP", g_load_error); return -1; }
  if (g_handle) return 0;
  /* ND4HIP_DEVICES = "all" | "0,1,2,...": one handle over several GPUs; batched calls on host arrays are then sharded along the
     leading batch axis (include/nd4hip.h, nd4hip_create_multi). Default: the single device ND4HIP_DEVICE (0). */
  const char* list = getenv("ND4HIP_DEVICES");
  if (list && *list) {
    int ids[64], n = 0;
    if (strcmp(list, "all") == 0) { const int cnt = p_device_count(); for (; n < cnt && n < 64; n++) ids[n] = n; }
    else for (const char* q = list; *q && n < 64;) { ids[n++] = atoi(q); while (*q && *q != ',') q++; if (*q == ',') q++; }
    if (n == 0) { napi_throw_error(env, "ND4HIP", "nd4hip: no HIP device available (ND4HIP_DEVICES)"); return -1; }
    if (p_create_multi(&g_handle, ids, n) != 0) { napi_throw_error(env, "ND4HIP", p_last_error()); g_handle = NULL; return -1; }
    return 0;
  }
  int dev = 0;
  const char* e = getenv("ND4HIP_DEVICE");
  if (e && *e) dev = atoi(e);
  if (p_create(&g_handle, dev) != 0) { napi_throw_error(env, "ND4HIP", p_last_error()); g_handle = NULL; return -1; }
  return 0;
}

static int get_i64(napi_env env, napi_value v, int64_t* out) {
  double d;
  if (napi_get_value_double(env, v, &d) != napi_ok) { napi_throw_type_error(env, "ND4HIP", "expected a number"); return -1; }
  *out = (int64_t)d;
  return 0;
}
/* typed array -> pointer + element count; `want` = napi_float64_array or napi_int32_array */
static int get_ta(napi_env env, napi_value v, napi_typedarray_type want, void** data, size_t* len) {
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (!is_ta) { napi_throw_type_error(env, "ND4HIP", "expected a TypedArray"); return -1; }
  napi_typedarray_type type; napi_value buf; size_t off;
  if (napi_get_typedarray_info(env, v, &type, len, data, &buf, &off) != napi_ok || type != want) {
    napi_throw_type_error(env, "ND4HIP", want == napi_float64_array ? "expected a Float64Array" : "expected an Int32Array");
    return -1;
  }
  return 0;
}

/* ---- device buffers: an external with a finalizer; JS passes views {b: buffer, o: element offset} ---- */
#define DEVBUF_MAGIC 0x6e64346869706466ull
typedef struct { uint64_t magic; void* p; size_t bytes; } devbuf;

static void devbuf_release(devbuf* b) {
  if (b->p && g_handle && p_free) p_free(g_handle, b->p);     /* after the env cleanup hook the handle (and its memory) is gone */
  b->p = NULL;
}
static void devbuf_finalize(napi_env env, void* data, void* hint) {
  (void)hint;
  devbuf* b = (devbuf*)data;
  if (b->p) { int64_t adj; napi_adjust_external_memory(env, -(int64_t)b->bytes, &adj); }
  devbuf_release(b);
  free(b);
}
static devbuf* get_devbuf(napi_env env, napi_value v) {
  napi_valuetype t;
  void* data = NULL;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_external || napi_get_value_external(env, v, &data) != napi_ok ||
      !data || ((devbuf*)data)->magic != DEVBUF_MAGIC) {
    napi_throw_type_error(env, "ND4HIP", "expected a device buffer from dev_alloc()");
    return NULL;
  }
  return (devbuf*)data;
}

/* one array operand: host TypedArray, or device view {b, o}; len = elements available from p */
typedef struct { void* p; size_t len; int dev; } opnd;
static int get_op(napi_env env, napi_value v, napi_typedarray_type want, opnd* out) {
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (is_ta) { out->dev = 0; return get_ta(env, v, want, &out->p, &out->len); }
  napi_valuetype t;
  napi_value vb, vo;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_object || napi_get_named_property(env, v, "b", &vb) != napi_ok ||
      napi_get_named_property(env, v, "o", &vo) != napi_ok) {
    napi_throw_type_error(env, "ND4HIP", "expected a TypedArray or a device view {b, o}");
    return -1;
  }
  devbuf* b = get_devbuf(env, vb);
  if (!b) return -1;
  if (!b->p) { napi_throw_error(env, "ND4HIP", "device buffer was already freed"); return -1; }
  int64_t off;
  if (get_i64(env, vo, &off)) return -1;
  const size_t esz = want == napi_float64_array ? 8 : 4, total = b->bytes / esz;
  if (off < 0 || (size_t)off > total) { napi_throw_range_error(env, "ND4HIP", "device view offset out of range"); return -1; }
  out->p = (char*)b->p + (size_t)off * esz;
  out->len = total - (size_t)off;
  out->dev = 1;
  return 0;
}
#define SAME_SIDE(cond, name) do { if (!(cond)) { napi_throw_type_error(env, "ND4HIP", name ": operands must be all host TypedArrays or all device views"); return NULL; } } while (0)

#define NEED(cond, msg) do { if (!(cond)) { napi_throw_range_error(env, "ND4HIP", msg); return NULL; } } while (0)

static napi_value js_device_count(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value r;
  if (load_library() != 0) THROW(env, g_load_error);
  napi_create_int32(env, p_device_count(), &r);
  return r;
}
/* devices() -> [ids] behind the (lazily created) handle */
static napi_value js_devices(napi_env env, napi_callback_info info) {
  (void)info;
  if (ensure_handle(env)) return NULL;
  int ids[64];
  const int n = p_device_list(g_handle, ids, 64);
  napi_value arr, v;
  napi_create_array_with_length(env, (size_t)n, &arr);
  for (int i = 0; i < n && i < 64; i++) { napi_create_int32(env, ids[i], &v); napi_set_element(env, arr, (uint32_t)i, v); }
  return arr;
}
static napi_value js_version(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value r;
  if (load_library() != 0) THROW(env, g_load_error);
  napi_create_string_utf8(env, p_version(), NAPI_AUTO_LENGTH, &r);
  return r;
}

#define ARGS(n, name) size_t argc = (n); napi_value a[(n)]; napi_get_cb_info(env, info, &argc, a, NULL, NULL); \
  NEED(argc == (n), name ": " #n " arguments expected")
#define F64(i, o) get_op(env, a[i], napi_float64_array, &(o))
#define I32(i, o) get_op(env, a[i], napi_int32_array, &(o))
#define FAIL_IF(rc) do { if ((rc) != 0) THROW(env, p_last_error()); } while (0)

/* dgemm_batched(batch, I, K, J, A, strideA, B, strideB, C) */
static napi_value js_dgemm(napi_env env, napi_callback_info info) {
  ARGS(9, "dgemm_batched");
  int64_t batch, I, K, J, sA, sB; opnd A, B, C;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &I) || get_i64(env, a[2], &K) || get_i64(env, a[3], &J) ||
      F64(4, A) || get_i64(env, a[5], &sA) || F64(6, B) || get_i64(env, a[7], &sB) || F64(8, C)) return NULL;
  NEED(batch >= 0 && I >= 0 && K >= 0 && J >= 0 && sA >= 0 && sB >= 0, "dgemm_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sA + I * K) <= A.len && (size_t)((batch - 1) * sB + K * J) <= B.len && (size_t)(batch * I * J) <= C.len),
       "dgemm_batched: buffer too small");
  SAME_SIDE(A.dev == B.dev && B.dev == C.dev, "dgemm_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgemm[A.dev](g_handle, batch, I, K, J, (const double*)A.p, sA, (const double*)B.p, sB, (double*)C.p));
  return NULL;
}
/* zgemm_batched(a_complex, b_complex, batch, I, K, J, A, strideA, B, strideB, C): complex operands are Float64Arrays (or
   device views) of interleaved (re, im) pairs, the reference's ComplexArray._array; extents and strides count elements, so a
   complex operand needs 2 doubles per element. C is always complex. */
static napi_value js_zgemm(napi_env env, napi_callback_info info) {
  ARGS(11, "zgemm_batched");
  int64_t ac, bc, batch, I, K, J, sA, sB; opnd A, B, C;
  if (get_i64(env, a[0], &ac) || get_i64(env, a[1], &bc) || get_i64(env, a[2], &batch) || get_i64(env, a[3], &I) ||
      get_i64(env, a[4], &K) || get_i64(env, a[5], &J) || F64(6, A) || get_i64(env, a[7], &sA) || F64(8, B) ||
      get_i64(env, a[9], &sB) || F64(10, C)) return NULL;
  NEED(ac || bc, "zgemm_batched: at least one operand must be complex");
  NEED(batch >= 0 && I >= 0 && K >= 0 && J >= 0 && sA >= 0 && sB >= 0, "zgemm_batched: negative extent");
  const size_t ea = ac ? 2 : 1, eb = bc ? 2 : 1;
  NEED(batch == 0 || (ea * (size_t)((batch - 1) * sA + I * K) <= A.len && eb * (size_t)((batch - 1) * sB + K * J) <= B.len &&
                      2 * (size_t)(batch * I * J) <= C.len),
       "zgemm_batched: buffer too small");
  SAME_SIDE(A.dev == B.dev && B.dev == C.dev, "zgemm_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zgemm[A.dev](g_handle, ac != 0, bc != 0, batch, I, K, J, (const double*)A.p, sA, (const double*)B.p, sB, (double*)C.p));
  return NULL;
}
/* dgetrf_batched(batch, N, A, LU, P) */
static napi_value js_dgetrf(napi_env env, napi_callback_info info) {
  ARGS(5, "dgetrf_batched");
  int64_t batch, N; opnd A, LU, P;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, A) || F64(3, LU) || I32(4, P)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= A.len && (size_t)(batch * N * N) <= LU.len && (size_t)(batch * N) <= P.len,
       "dgetrf_batched: buffer too small");
  SAME_SIDE(A.dev == LU.dev && LU.dev == P.dev, "dgetrf_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgetrf[A.dev](g_handle, batch, N, (const double*)A.p, (double*)LU.p, (int32_t*)P.p));
  return NULL;
}
/* dgeqrf_q_batched(batch, M, N, A, Q, R) */
static napi_value js_dgeqrf(napi_env env, napi_callback_info info) {
  ARGS(6, "dgeqrf_q_batched");
  int64_t batch, M, N; opnd A, Q, R;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, Q) || F64(5, R)) return NULL;
  int64_t L = M < N ? M : N;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * L) <= Q.len && (size_t)(batch * L * N) <= R.len,
       "dgeqrf_q_batched: buffer too small");
  SAME_SIDE(A.dev == Q.dev && Q.dev == R.dev, "dgeqrf_q_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgeqrf[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)Q.p, (double*)R.p));
  return NULL;
}
/* dgeqrf_full_batched(batch, M, N, A, Q, R)   (qr_decomp_full, qr.js:27-77: Q is M x M, R is M x N) */
static napi_value js_dgeqrf_full(napi_env env, napi_callback_info info) {
  ARGS(6, "dgeqrf_full_batched");
  int64_t batch, M, N; opnd A, Q, R;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, Q) || F64(5, R)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * M) <= Q.len && (size_t)(batch * M * N) <= R.len,
       "dgeqrf_full_batched: buffer too small");
  SAME_SIDE(A.dev == Q.dev && Q.dev == R.dev, "dgeqrf_full_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgeqrf_full[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)Q.p, (double*)R.p));
  return NULL;
}
/* dgeqrf_qty_batched(batch, M, N, L, A, Y)   (_qr_decomp_inplace, qr.js:146-183: A <- R, Y <- Q^T Y in place) */
static napi_value js_dgeqrf_qty(napi_env env, napi_callback_info info) {
  ARGS(6, "dgeqrf_qty_batched");
  int64_t batch, M, N, L; opnd A, Y;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || get_i64(env, a[3], &L) || F64(4, A) || F64(5, Y)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && L >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * L) <= Y.len,
       "dgeqrf_qty_batched: buffer too small");
  SAME_SIDE(A.dev == Y.dev, "dgeqrf_qty_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgeqrf_qty[A.dev](g_handle, batch, M, N, L, (double*)A.p, (double*)Y.p));
  return NULL;
}
/* dgebrd_batched(batch, M, N, A, U, B, V)   (bidiag_decomp, bidiag.js:245-319) */
static napi_value js_dgebrd(napi_env env, napi_callback_info info) {
  ARGS(7, "dgebrd_batched");
  int64_t batch, M, N; opnd A, U, B, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, U) || F64(5, B) || F64(6, V)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0, "dgebrd_batched: negative extent");
  const int64_t K = M < N ? M : N, J = M >= N ? K : K + 1;
  NEED((size_t)(batch * M * N) <= A.len && (size_t)(batch * M * K) <= U.len && (size_t)(batch * K * J) <= B.len && (size_t)(batch * J * N) <= V.len,
       "dgebrd_batched: buffer too small");
  SAME_SIDE(A.dev == U.dev && U.dev == B.dev && B.dev == V.dev, "dgebrd_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgebrd[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)U.p, (double*)B.p, (double*)V.p));
  return NULL;
}
/* dgehrd_batched(batch, N, A, U, H)   (hessenberg_decomp, hessenberg.js:89-115) */
static napi_value js_dgehrd(napi_env env, napi_callback_info info) {
  ARGS(5, "dgehrd_batched");
  int64_t batch, N; opnd A, U, H;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, A) || F64(3, U) || F64(4, H)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= A.len && (size_t)(batch * N * N) <= U.len && (size_t)(batch * N * N) <= H.len,
       "dgehrd_batched: buffer too small");
  SAME_SIDE(A.dev == U.dev && U.dev == H.dev, "dgehrd_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgehrd[A.dev](g_handle, batch, N, (const double*)A.p, (double*)U.p, (double*)H.p));
  return NULL;
}
/* dgesvdj_batched(batch, M, N, A, U, sv, V) -> {sweeps, offnorm, rotations} */
static napi_value js_dgesvdj(napi_env env, napi_callback_info info) {
  ARGS(7, "dgesvdj_batched");
  int64_t batch, M, N; opnd A, U, S, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, U) || F64(5, S) || F64(6, V)) return NULL;
  int64_t L = M < N ? M : N;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * L) <= U.len &&
       (size_t)(batch * L) <= S.len && (size_t)(batch * L * N) <= V.len, "dgesvdj_batched: buffer too small");
  SAME_SIDE(A.dev == U.dev && U.dev == S.dev && S.dev == V.dev, "dgesvdj_batched");
  if (ensure_handle(env)) return NULL;
  int sweeps = 0; double off = 0.0;
  FAIL_IF(p_dgesvdj[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)U.p, (double*)S.p, (double*)V.p, &sweeps, &off));
  napi_value r, v;
  napi_create_object(env, &r);
  napi_create_int32(env, sweeps, &v); napi_set_named_property(env, r, "sweeps", v);
  napi_create_double(env, off, &v); napi_set_named_property(env, r, "offnorm", v);
  unsigned long long rot = 0;
  FAIL_IF(p_svd_info(g_handle, NULL, &rot, NULL));
  napi_create_double(env, (double)rot, &v); napi_set_named_property(env, r, "rotations", v);     /* exact up to 2^53 */
  return r;
}
/* dgesdd_batched(batch, M, N, A, U, sv, V)   (svd_decomp by divide & conquer, svd_dc.js:883-932) */
static napi_value js_dgesdd(napi_env env, napi_callback_info info) {
  ARGS(7, "dgesdd_batched");
  int64_t batch, M, N; opnd A, U, S, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, U) || F64(5, S) || F64(6, V)) return NULL;
  int64_t L = M < N ? M : N;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * L) <= U.len &&
       (size_t)(batch * L) <= S.len && (size_t)(batch * L * N) <= V.len, "dgesdd_batched: buffer too small");
  SAME_SIDE(A.dev == U.dev && U.dev == S.dev && S.dev == V.dev, "dgesdd_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgesdd[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)U.p, (double*)S.p, (double*)V.p));
  return NULL;
}

/* dgetrs_batched(batch, N, J, LU, strideLU, P, strideP, Y, strideY, X)   (lu_solve, lu.js:84-177) */
static napi_value js_dgetrs(napi_env env, napi_callback_info info) {
  ARGS(10, "dgetrs_batched");
  int64_t batch, N, J, sLU, sP, sY; opnd LU, P, Y, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &J) || F64(3, LU) || get_i64(env, a[4], &sLU) ||
      I32(5, P) || get_i64(env, a[6], &sP) || F64(7, Y) || get_i64(env, a[8], &sY) || F64(9, X)) return NULL;
  NEED(batch >= 0 && N >= 0 && J >= 0 && sLU >= 0 && sP >= 0 && sY >= 0, "dgetrs_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sLU + N * N) <= LU.len && (size_t)((batch - 1) * sP + N) <= P.len &&
                      (size_t)((batch - 1) * sY + N * J) <= Y.len && (size_t)(batch * N * J) <= X.len), "dgetrs_batched: buffer too small");
  SAME_SIDE(LU.dev == P.dev && P.dev == Y.dev && Y.dev == X.dev, "dgetrs_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgetrs[X.dev](g_handle, batch, N, J, (const double*)LU.p, sLU, (const int32_t*)P.p, sP, (const double*)Y.p, sY, (double*)X.p));
  return NULL;
}
/* dtrsm_batched(upper, unit_diag, batch, M, J, T, strideT, Y, strideY, X)   (tril_solve / triu_solve, tri.js:155-290) */
static napi_value js_dtrsm(napi_env env, napi_callback_info info) {
  ARGS(10, "dtrsm_batched");
  int64_t upper, unit, batch, M, J, sT, sY; opnd T, Y, X;
  if (get_i64(env, a[0], &upper) || get_i64(env, a[1], &unit) || get_i64(env, a[2], &batch) || get_i64(env, a[3], &M) || get_i64(env, a[4], &J) ||
      F64(5, T) || get_i64(env, a[6], &sT) || F64(7, Y) || get_i64(env, a[8], &sY) || F64(9, X)) return NULL;
  NEED(batch >= 0 && M >= 0 && J >= 0 && sT >= 0 && sY >= 0, "dtrsm_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sT + M * M) <= T.len && (size_t)((batch - 1) * sY + M * J) <= Y.len && (size_t)(batch * M * J) <= X.len),
       "dtrsm_batched: buffer too small");
  SAME_SIDE(T.dev == Y.dev && Y.dev == X.dev, "dtrsm_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dtrsm[X.dev](g_handle, (int)upper, (int)unit, batch, M, J, (const double*)T.p, sT, (const double*)Y.p, sY, (double*)X.p));
  return NULL;
}
/* dqrls_batched(batch, N, M, I, J, Q, strideQ, R, strideR, Y, strideY, X)   (qr_lstsq, qr.js:186-273) */
static napi_value js_dqrls(napi_env env, napi_callback_info info) {
  ARGS(12, "dqrls_batched");
  int64_t batch, N, M, I, J, sQ, sR, sY; opnd Q, R, Y, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &M) || get_i64(env, a[3], &I) || get_i64(env, a[4], &J) ||
      F64(5, Q) || get_i64(env, a[6], &sQ) || F64(7, R) || get_i64(env, a[8], &sR) || F64(9, Y) || get_i64(env, a[10], &sY) || F64(11, X)) return NULL;
  NEED(batch >= 0 && N >= 0 && M >= 0 && I >= 0 && J >= 0 && sQ >= 0 && sR >= 0 && sY >= 0, "dqrls_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sQ + N * M) <= Q.len && (size_t)((batch - 1) * sR + M * I) <= R.len &&
                      (size_t)((batch - 1) * sY + N * J) <= Y.len && (size_t)(batch * I * J) <= X.len), "dqrls_batched: buffer too small");
  SAME_SIDE(Q.dev == R.dev && R.dev == Y.dev && Y.dev == X.dev, "dqrls_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dqrls[X.dev](g_handle, batch, N, M, I, J, (const double*)Q.p, sQ, (const double*)R.p, sR, (const double*)Y.p, sY, (double*)X.p));
  return NULL;
}
/* dgeqp3_batched / dgeqp3_full_batched(batch, M, N, A, Q, R, P)   (rrqr_decomp, rrqr.js:278-395 / rrqr_decomp_full :88-184) */
static napi_value geqp3_common(napi_env env, napi_callback_info info, int full) {
  size_t argc = 7; napi_value a[7]; napi_get_cb_info(env, info, &argc, a, NULL, NULL);
  NEED(argc == 7, "dgeqp3_batched: 7 arguments expected");
  int64_t batch, M, N; opnd A, Q, R, P;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, Q) || F64(5, R) || I32(6, P)) return NULL;
  const int64_t L = M < N ? M : N, qc = full ? M : L, rr = full ? M : L;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * qc) <= Q.len &&
       (size_t)(batch * rr * N) <= R.len && (size_t)(batch * N) <= P.len, "dgeqp3_batched: buffer too small");
  SAME_SIDE(A.dev == Q.dev && Q.dev == R.dev && R.dev == P.dev, "dgeqp3_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF((full ? p_dgeqp3_full : p_dgeqp3)[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)Q.p, (double*)R.p, (int32_t*)P.p));
  return NULL;
}
static napi_value js_dgeqp3(napi_env env, napi_callback_info info) { return geqp3_common(env, info, 0); }
static napi_value js_dgeqp3_full(napi_env env, napi_callback_info info) { return geqp3_common(env, info, 1); }
/* dsrrqr_batched(batch, M, N, A, dtol, ztol, Q, R, P, rank)   (srrqr_decomp_full, srrqr.js:58-802; ztol < 0: the default) */
static napi_value js_dsrrqr(napi_env env, napi_callback_info info) {
  ARGS(10, "dsrrqr_batched");
  int64_t batch, M, N; double dtol, ztol; opnd A, Q, R, P, r;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) ||
      napi_get_value_double(env, a[4], &dtol) != napi_ok || napi_get_value_double(env, a[5], &ztol) != napi_ok ||
      F64(6, Q) || F64(7, R) || I32(8, P) || I32(9, r)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * M) <= Q.len &&
       (size_t)(batch * M * N) <= R.len && (size_t)(batch * N) <= P.len && (size_t)batch <= r.len, "dsrrqr_batched: buffer too small");
  SAME_SIDE(A.dev == Q.dev && Q.dev == R.dev && R.dev == P.dev && P.dev == r.dev, "dsrrqr_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsrrqr[A.dev](g_handle, batch, M, N, (const double*)A.p, dtol, ztol, (double*)Q.p, (double*)R.p, (int32_t*)P.p, (int32_t*)r.p));
  return NULL;
}
/* durv_batched(batch, M, N, A, U, R, V, rank)   (urv_decomp_full, urv.js:100-135) */
static napi_value js_durv(napi_env env, napi_callback_info info) {
  ARGS(8, "durv_batched");
  int64_t batch, M, N; opnd A, U, R, V, r;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, U) || F64(5, R) || F64(6, V) ||
      I32(7, r)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * M) <= U.len && (size_t)(batch * M * N) <= R.len &&
       (size_t)(batch * N * N) <= V.len && (size_t)batch <= r.len, "durv_batched: buffer too small");
  SAME_SIDE(A.dev == U.dev && U.dev == R.dev && R.dev == V.dev && V.dev == r.dev, "durv_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_durv[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)U.p, (double*)R.p, (double*)V.p, (int32_t*)r.p));
  return NULL;
}
/* durvls_batched(batch, I, J, K, L, Jc, U, sU, R, sR, V, sV, rank, sRank, Y, sY, X)   (urv_lstsq, urv.js:138-323) */
static napi_value js_durvls(napi_env env, napi_callback_info info) {
  ARGS(17, "durvls_batched");
  int64_t batch, I, J, K, L, Jc, sU, sR, sV, sK, sY; opnd U, R, V, k, Y, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &I) || get_i64(env, a[2], &J) || get_i64(env, a[3], &K) || get_i64(env, a[4], &L) ||
      get_i64(env, a[5], &Jc) || F64(6, U) || get_i64(env, a[7], &sU) || F64(8, R) || get_i64(env, a[9], &sR) || F64(10, V) ||
      get_i64(env, a[11], &sV) || I32(12, k) || get_i64(env, a[13], &sK) || F64(14, Y) || get_i64(env, a[15], &sY) || F64(16, X)) return NULL;
  NEED(batch >= 0 && I >= 0 && J >= 0 && K >= 0 && L >= 0 && Jc >= 0 && sU >= 0 && sR >= 0 && sV >= 0 && sK >= 0 && sY >= 0,
       "durvls_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sU + I * J) <= U.len && (size_t)((batch - 1) * sR + J * K) <= R.len &&
                      (size_t)((batch - 1) * sV + K * L) <= V.len && (size_t)((batch - 1) * sK + 1) <= k.len &&
                      (size_t)((batch - 1) * sY + I * Jc) <= Y.len && (size_t)(batch * L * Jc) <= X.len), "durvls_batched: buffer too small");
  SAME_SIDE(U.dev == R.dev && R.dev == V.dev && V.dev == k.dev && k.dev == Y.dev && Y.dev == X.dev, "durvls_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_durvls[X.dev](g_handle, batch, I, J, K, L, Jc, (const double*)U.p, sU, (const double*)R.p, sR, (const double*)V.p, sV,
                          (const int32_t*)k.p, sK, (const double*)Y.p, sY, (double*)X.p));
  return NULL;
}
/* ddet_batched(batch, M, N, A, det) / dslogdet_batched(batch, M, N, A, sign, logdet)   (det / slogdet, det.js:95-106) */
static napi_value js_ddet(napi_env env, napi_callback_info info) {
  ARGS(5, "ddet_batched");
  int64_t batch, M, N; opnd A, D;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, D)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)batch <= D.len, "ddet_batched: buffer too small");
  SAME_SIDE(A.dev == D.dev, "ddet_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_ddet[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)D.p));
  return NULL;
}
static napi_value js_dslogdet(napi_env env, napi_callback_info info) {
  ARGS(6, "dslogdet_batched");
  int64_t batch, M, N; opnd A, S, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, S) || F64(5, L)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)batch <= S.len && (size_t)batch <= L.len,
       "dslogdet_batched: buffer too small");
  SAME_SIDE(A.dev == S.dev && S.dev == L.dev, "dslogdet_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dslogdet[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)S.p, (double*)L.p));
  return NULL;
}
/* ddettri_batched(batch, N, A, det) / dslogdettri_batched(batch, N, A, sign, logdet)   (det_tri / slogdet_tri, det.js:24-92) */
static napi_value js_ddettri(napi_env env, napi_callback_info info) {
  ARGS(4, "ddettri_batched");
  int64_t batch, N; opnd A, D;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, A) || F64(3, D)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= A.len && (size_t)batch <= D.len, "ddettri_batched: buffer too small");
  SAME_SIDE(A.dev == D.dev, "ddettri_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_ddettri[A.dev](g_handle, batch, N, (const double*)A.p, (double*)D.p));
  return NULL;
}
static napi_value js_dslogdettri(napi_env env, napi_callback_info info) {
  ARGS(5, "dslogdettri_batched");
  int64_t batch, N; opnd A, S, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, A) || F64(3, S) || F64(4, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= A.len && (size_t)batch <= S.len && (size_t)batch <= L.len,
       "dslogdettri_batched: buffer too small");
  SAME_SIDE(A.dev == S.dev && S.dev == L.dev, "dslogdettri_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dslogdettri[A.dev](g_handle, batch, N, (const double*)A.p, (double*)S.p, (double*)L.p));
  return NULL;
}
/* dtreval_batched(batch, N, T, Lam) / dtrevc_batched(batch, N, Q, T, Lam, V)   (schur_eigenvals / schur_eigen, schur.js:31-370);
 * Lam and V are complex: Float64Arrays (or device views) of interleaved (re, im) doubles */
static napi_value js_dtreval(napi_env env, napi_callback_info info) {
  ARGS(4, "dtreval_batched");
  int64_t batch, N; opnd T, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, T) || F64(3, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= T.len && (size_t)(2 * batch * N) <= L.len, "dtreval_batched: buffer too small");
  SAME_SIDE(T.dev == L.dev, "dtreval_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dtreval[T.dev](g_handle, batch, N, (const double*)T.p, (double*)L.p));
  return NULL;
}
static napi_value js_dtrevc(napi_env env, napi_callback_info info) {
  ARGS(6, "dtrevc_batched");
  int64_t batch, N; opnd Q, T, L, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, Q) || F64(3, T) || F64(4, L) || F64(5, V)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= Q.len && (size_t)(batch * N * N) <= T.len && (size_t)(2 * batch * N) <= L.len &&
       (size_t)(2 * batch * N * N) <= V.len, "dtrevc_batched: buffer too small");
  SAME_SIDE(Q.dev == T.dev && T.dev == L.dev && L.dev == V.dev, "dtrevc_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dtrevc[T.dev](g_handle, batch, N, (const double*)Q.p, (const double*)T.p, (double*)L.p, (double*)V.p));
  return NULL;
}
/* dgebal_batched(batch, N, p, A, D, B) / zgebak_batched(batch, N, D, V, W)   (eigen_balance_pre / _post, eigen.js:91-270); V, W complex */
static napi_value js_dgebal(napi_env env, napi_callback_info info) {
  ARGS(6, "dgebal_batched");
  int64_t batch, N; double p; opnd A, D, B;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || napi_get_value_double(env, a[2], &p) != napi_ok || F64(3, A) || F64(4, D) || F64(5, B)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= A.len && (size_t)(batch * N) <= D.len && (size_t)(batch * N * N) <= B.len,
       "dgebal_batched: buffer too small");
  SAME_SIDE(A.dev == D.dev && D.dev == B.dev, "dgebal_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgebal[A.dev](g_handle, batch, N, p, (const double*)A.p, (double*)D.p, (double*)B.p));
  return NULL;
}
static napi_value js_zgebak(napi_env env, napi_callback_info info) {
  ARGS(5, "zgebak_batched");
  int64_t batch, N; opnd D, V, W;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, D) || F64(3, V) || F64(4, W)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N) <= D.len && (size_t)(2 * batch * N * N) <= V.len && (size_t)(2 * batch * N * N) <= W.len,
       "zgebak_batched: buffer too small");
  SAME_SIDE(D.dev == V.dev && V.dev == W.dev, "zgebak_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zgebak[D.dev](g_handle, batch, N, (const double*)D.p, (const double*)V.p, (double*)W.p));
  return NULL;
}
/* dhseqr_batched(batch, N, U, H, Q, T) / dgees_batched(batch, N, A, Q, T) -> the most sweeps of one francis_qr call
 * (schur_qrfrancis_inplace / schur_decomp, schur.js:372-683); dgeev_batched(batch, N, A, Lam, V) / dgeevals_batched(batch, N, A, Lam)
 * (eigen / eigenvals, eigen.js:33-88); Lam and V complex */
static napi_value js_dhseqr(napi_env env, napi_callback_info info) {
  ARGS(6, "dhseqr_batched");
  int64_t batch, N; opnd U, H, Q, T;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, U) || F64(3, H) || F64(4, Q) || F64(5, T)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= U.len && (size_t)(batch * N * N) <= H.len && (size_t)(batch * N * N) <= Q.len &&
       (size_t)(batch * N * N) <= T.len, "dhseqr_batched: buffer too small");
  SAME_SIDE(U.dev == H.dev && H.dev == Q.dev && Q.dev == T.dev, "dhseqr_batched");
  if (ensure_handle(env)) return NULL;
  int sweeps = 0;
  FAIL_IF(p_dhseqr[U.dev](g_handle, batch, N, (const double*)U.p, (const double*)H.p, (double*)Q.p, (double*)T.p, &sweeps));
  napi_value out;
  napi_create_int32(env, sweeps, &out);
  return out;
}
static napi_value js_dgees(napi_env env, napi_callback_info info) {
  ARGS(5, "dgees_batched");
  int64_t batch, N; opnd A, Q, T;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, A) || F64(3, Q) || F64(4, T)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= A.len && (size_t)(batch * N * N) <= Q.len && (size_t)(batch * N * N) <= T.len,
       "dgees_batched: buffer too small");
  SAME_SIDE(A.dev == Q.dev && Q.dev == T.dev, "dgees_batched");
  if (ensure_handle(env)) return NULL;
  int sweeps = 0;
  FAIL_IF(p_dgees[A.dev](g_handle, batch, N, (const double*)A.p, (double*)Q.p, (double*)T.p, &sweeps));
  napi_value out;
  napi_create_int32(env, sweeps, &out);
  return out;
}
static napi_value js_dgeev(napi_env env, napi_callback_info info) {
  ARGS(5, "dgeev_batched");
  int64_t batch, N; opnd A, L, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, A) || F64(3, L) || F64(4, V)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= A.len && (size_t)(2 * batch * N) <= L.len && (size_t)(2 * batch * N * N) <= V.len,
       "dgeev_batched: buffer too small");
  SAME_SIDE(A.dev == L.dev && L.dev == V.dev, "dgeev_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgeev[A.dev](g_handle, batch, N, (const double*)A.p, (double*)L.p, (double*)V.p));
  return NULL;
}
static napi_value js_dgeevals(napi_env env, napi_callback_info info) {
  ARGS(4, "dgeevals_batched");
  int64_t batch, N; opnd A, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, A) || F64(3, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= A.len && (size_t)(2 * batch * N) <= L.len, "dgeevals_batched: buffer too small");
  SAME_SIDE(A.dev == L.dev, "dgeevals_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgeev[A.dev](g_handle, batch, N, (const double*)A.p, (double*)L.p, NULL));
  return NULL;
}
/* dsyevd_batched(batch, N, S, L, V) / dsyevals_batched(batch, N, S, L)   (eigen_sym / eigenvals_sym, planned at eigen.js:28-30) */
static napi_value js_dsyevd(napi_env env, napi_callback_info info) {
  ARGS(5, "dsyevd_batched");
  int64_t batch, N; opnd S, L, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, S) || F64(3, L) || F64(4, V)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= S.len && (size_t)(batch * N) <= L.len && (size_t)(batch * N * N) <= V.len,
       "dsyevd_batched: buffer too small");
  SAME_SIDE(S.dev == L.dev && L.dev == V.dev, "dsyevd_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevd[S.dev](g_handle, batch, N, (const double*)S.p, (double*)L.p, (double*)V.p));
  return NULL;
}
static napi_value js_dsyevals(napi_env env, napi_callback_info info) {
  ARGS(4, "dsyevals_batched");
  int64_t batch, N; opnd S, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, S) || F64(3, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= S.len && (size_t)(batch * N) <= L.len, "dsyevals_batched: buffer too small");
  SAME_SIDE(S.dev == L.dev, "dsyevals_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevd[S.dev](g_handle, batch, N, (const double*)S.p, (double*)L.p, NULL));
  return NULL;
}
/* dsyevj_batched(batch, N, S, L, V) / dsyevjals_batched(batch, N, S, L)   (eigen_sym / eigenvals_sym with {algo: 'jacobi'}, N <= 128;
 * the sweep counts are not asked for) */
static napi_value js_dsyevj(napi_env env, napi_callback_info info) {
  ARGS(5, "dsyevj_batched");
  int64_t batch, N; opnd S, L, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, S) || F64(3, L) || F64(4, V)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= S.len && (size_t)(batch * N) <= L.len && (size_t)(batch * N * N) <= V.len,
       "dsyevj_batched: buffer too small");
  SAME_SIDE(S.dev == L.dev && L.dev == V.dev, "dsyevj_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevj[S.dev](g_handle, batch, N, (const double*)S.p, (double*)L.p, (double*)V.p, NULL));
  return NULL;
}
static napi_value js_dsyevjals(napi_env env, napi_callback_info info) {
  ARGS(4, "dsyevjals_batched");
  int64_t batch, N; opnd S, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, S) || F64(3, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= S.len && (size_t)(batch * N) <= L.len, "dsyevjals_batched: buffer too small");
  SAME_SIDE(S.dev == L.dev, "dsyevjals_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevj[S.dev](g_handle, batch, N, (const double*)S.p, (double*)L.p, NULL, NULL));
  return NULL;
}
/* dsyevx_batched(batch, N, i0, i1, S, L, V) / dsyevxals_batched(batch, N, i0, i1, S, L)   (eigen_sym / eigenvals_sym with
 * {subset: [i0, i1]}: L [batch, i1 - i0], V [batch, N, i1 - i0]; the subset itself is checked by the library) */
static napi_value js_dsyevx(napi_env env, napi_callback_info info) {
  ARGS(7, "dsyevx_batched");
  int64_t batch, N, i0, i1; opnd S, L, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &i0) || get_i64(env, a[3], &i1) || F64(4, S) || F64(5, L) ||
      F64(6, V)) return NULL;
  NEED(batch >= 0 && N >= 0 && 0 <= i0 && i0 <= i1 && i1 <= N && (size_t)(batch * N * N) <= S.len && (size_t)(batch * (i1 - i0)) <= L.len &&
       (size_t)(batch * N * (i1 - i0)) <= V.len, "dsyevx_batched: bad subset or buffer too small");
  SAME_SIDE(S.dev == L.dev && L.dev == V.dev, "dsyevx_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevx[S.dev](g_handle, batch, N, i0, i1, (const double*)S.p, (double*)L.p, (double*)V.p));
  return NULL;
}
static napi_value js_dsyevxals(napi_env env, napi_callback_info info) {
  ARGS(6, "dsyevxals_batched");
  int64_t batch, N, i0, i1; opnd S, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &i0) || get_i64(env, a[3], &i1) || F64(4, S) || F64(5, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && 0 <= i0 && i0 <= i1 && i1 <= N && (size_t)(batch * N * N) <= S.len && (size_t)(batch * (i1 - i0)) <= L.len,
       "dsyevxals_batched: bad subset or buffer too small");
  SAME_SIDE(S.dev == L.dev, "dsyevxals_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevx[S.dev](g_handle, batch, N, i0, i1, (const double*)S.p, (double*)L.p, NULL));
  return NULL;
}
/* dsyevd_tr_batched / dsyevdals_tr_batched / dsyevx_tr_batched / dsyevxals_tr_batched: the four calls above with {reduction:
 * 'tridiag'} (csrc/sytrd.hip), the same argument lists */
static napi_value js_dsyevd_tr(napi_env env, napi_callback_info info) {
  ARGS(5, "dsyevd_tr_batched");
  int64_t batch, N; opnd S, L, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, S) || F64(3, L) || F64(4, V)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= S.len && (size_t)(batch * N) <= L.len && (size_t)(batch * N * N) <= V.len,
       "dsyevd_tr_batched: buffer too small");
  SAME_SIDE(S.dev == L.dev && L.dev == V.dev, "dsyevd_tr_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevd_tr[S.dev](g_handle, batch, N, (const double*)S.p, (double*)L.p, (double*)V.p));
  return NULL;
}
static napi_value js_dsyevdals_tr(napi_env env, napi_callback_info info) {
  ARGS(4, "dsyevdals_tr_batched");
  int64_t batch, N; opnd S, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, S) || F64(3, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= S.len && (size_t)(batch * N) <= L.len, "dsyevdals_tr_batched: buffer too small");
  SAME_SIDE(S.dev == L.dev, "dsyevdals_tr_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevd_tr[S.dev](g_handle, batch, N, (const double*)S.p, (double*)L.p, NULL));
  return NULL;
}
static napi_value js_dsyevx_tr(napi_env env, napi_callback_info info) {
  ARGS(7, "dsyevx_tr_batched");
  int64_t batch, N, i0, i1; opnd S, L, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &i0) || get_i64(env, a[3], &i1) || F64(4, S) || F64(5, L) ||
      F64(6, V)) return NULL;
  NEED(batch >= 0 && N >= 0 && 0 <= i0 && i0 <= i1 && i1 <= N && (size_t)(batch * N * N) <= S.len && (size_t)(batch * (i1 - i0)) <= L.len &&
       (size_t)(batch * N * (i1 - i0)) <= V.len, "dsyevx_tr_batched: bad subset or buffer too small");
  SAME_SIDE(S.dev == L.dev && L.dev == V.dev, "dsyevx_tr_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevx_tr[S.dev](g_handle, batch, N, i0, i1, (const double*)S.p, (double*)L.p, (double*)V.p));
  return NULL;
}
static napi_value js_dsyevxals_tr(napi_env env, napi_callback_info info) {
  ARGS(6, "dsyevxals_tr_batched");
  int64_t batch, N, i0, i1; opnd S, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &i0) || get_i64(env, a[3], &i1) || F64(4, S) || F64(5, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && 0 <= i0 && i0 <= i1 && i1 <= N && (size_t)(batch * N * N) <= S.len && (size_t)(batch * (i1 - i0)) <= L.len,
       "dsyevxals_tr_batched: bad subset or buffer too small");
  SAME_SIDE(S.dev == L.dev, "dsyevxals_tr_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevx_tr[S.dev](g_handle, batch, N, i0, i1, (const double*)S.p, (double*)L.p, NULL));
  return NULL;
}
/* zheevd_batched(batch, N, H, L, V) / zheevdals_batched(batch, N, H, L) / zheevx_batched(batch, N, i0, i1, H, L, V) /
 * zheevxals_batched(batch, N, i0, i1, H, L)   (eigen_herm / eigenvals_herm, csrc/hetrd.hip: H and V are complex128 as interleaved
 * doubles in Float64Arrays of twice the element count, L is real) */
static napi_value js_zheevd(napi_env env, napi_callback_info info) {
  ARGS(5, "zheevd_batched");
  int64_t batch, N; opnd H, L, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, H) || F64(3, L) || F64(4, V)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(2 * batch * N * N) <= H.len && (size_t)(batch * N) <= L.len && (size_t)(2 * batch * N * N) <= V.len,
       "zheevd_batched: buffer too small");
  SAME_SIDE(H.dev == L.dev && L.dev == V.dev, "zheevd_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zheevd[H.dev](g_handle, batch, N, (const double*)H.p, (double*)L.p, (double*)V.p));
  return NULL;
}
static napi_value js_zheevdals(napi_env env, napi_callback_info info) {
  ARGS(4, "zheevdals_batched");
  int64_t batch, N; opnd H, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, H) || F64(3, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(2 * batch * N * N) <= H.len && (size_t)(batch * N) <= L.len, "zheevdals_batched: buffer too small");
  SAME_SIDE(H.dev == L.dev, "zheevdals_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zheevd[H.dev](g_handle, batch, N, (const double*)H.p, (double*)L.p, NULL));
  return NULL;
}
static napi_value js_zheevx(napi_env env, napi_callback_info info) {
  ARGS(7, "zheevx_batched");
  int64_t batch, N, i0, i1; opnd H, L, V;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &i0) || get_i64(env, a[3], &i1) || F64(4, H) || F64(5, L) ||
      F64(6, V)) return NULL;
  NEED(batch >= 0 && N >= 0 && 0 <= i0 && i0 <= i1 && i1 <= N && (size_t)(2 * batch * N * N) <= H.len && (size_t)(batch * (i1 - i0)) <= L.len &&
       (size_t)(2 * batch * N * (i1 - i0)) <= V.len, "zheevx_batched: bad subset or buffer too small");
  SAME_SIDE(H.dev == L.dev && L.dev == V.dev, "zheevx_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zheevx[H.dev](g_handle, batch, N, i0, i1, (const double*)H.p, (double*)L.p, (double*)V.p));
  return NULL;
}
static napi_value js_zheevxals(napi_env env, napi_callback_info info) {
  ARGS(6, "zheevxals_batched");
  int64_t batch, N, i0, i1; opnd H, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &i0) || get_i64(env, a[3], &i1) || F64(4, H) || F64(5, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && 0 <= i0 && i0 <= i1 && i1 <= N && (size_t)(2 * batch * N * N) <= H.len && (size_t)(batch * (i1 - i0)) <= L.len,
       "zheevxals_batched: bad subset or buffer too small");
  SAME_SIDE(H.dev == L.dev, "zheevxals_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zheevx[H.dev](g_handle, batch, N, i0, i1, (const double*)H.p, (double*)L.p, NULL));
  return NULL;
}
/* zpotrf_batched(batch, N, H, L) / zpotrs_batched(batch, N, K, L, strideL, Y, X) / zhegvd_batched(batch, N, A, B, strideB, Lam, X) /
 * zhegvals_batched(batch, N, A, B, strideB, Lam) / zhegvx_batched(batch, N, i0, i1, A, B, strideB, Lam, X) / zhegvxals_batched(batch,
 * N, i0, i1, A, B, strideB, Lam)   (herm_cholesky_decomp / herm_cholesky_solve / eigen_herm_gen / eigenvals_herm_gen, csrc/hegv.hip:
 * H, L, Y, X, A and B are complex128 as interleaved doubles in Float64Arrays of twice the element count, Lam is real; strides
 * count complex elements, N*N or 0 = one L or B) */
static napi_value js_zpotrf(napi_env env, napi_callback_info info) {
  ARGS(4, "zpotrf_batched");
  int64_t batch, N; opnd H, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, H) || F64(3, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(2 * batch * N * N) <= H.len && (size_t)(2 * batch * N * N) <= L.len, "zpotrf_batched: buffer too small");
  SAME_SIDE(H.dev == L.dev, "zpotrf_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zpotrf[H.dev](g_handle, batch, N, (const double*)H.p, (double*)L.p));
  return NULL;
}
static napi_value js_zpotrs(napi_env env, napi_callback_info info) {
  ARGS(7, "zpotrs_batched");
  int64_t batch, N, K, sL; opnd L, Y, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &K) || F64(3, L) || get_i64(env, a[4], &sL) || F64(5, Y) ||
      F64(6, X)) return NULL;
  NEED(batch >= 0 && N >= 0 && K >= 0 && (sL == 0 || sL == N * N) && (size_t)(2 * (sL ? batch : 1) * N * N) <= L.len &&
       (size_t)(2 * batch * N * K) <= Y.len && (size_t)(2 * batch * N * K) <= X.len, "zpotrs_batched: buffer too small");
  SAME_SIDE(L.dev == Y.dev && Y.dev == X.dev, "zpotrs_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zpotrs[L.dev](g_handle, batch, N, K, (const double*)L.p, sL, (const double*)Y.p, (double*)X.p));
  return NULL;
}
#define ZHEGV_FITS(k) (batch >= 0 && N >= 0 && (sB == 0 || sB == N * N) && (size_t)(2 * batch * N * N) <= A.len && \
                       (size_t)(2 * (sB ? batch : 1) * N * N) <= B.len && (size_t)(batch * (k)) <= L.len)
static napi_value js_zhegvd(napi_env env, napi_callback_info info) {
  ARGS(7, "zhegvd_batched");
  int64_t batch, N, sB; opnd A, B, L, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, A) || F64(3, B) || get_i64(env, a[4], &sB) || F64(5, L) || F64(6, X)) return NULL;
  NEED(ZHEGV_FITS(N) && (size_t)(2 * batch * N * N) <= X.len, "zhegvd_batched: buffer too small");
  SAME_SIDE(A.dev == B.dev && B.dev == L.dev && L.dev == X.dev, "zhegvd_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zhegvd[A.dev](g_handle, batch, N, (const double*)A.p, (const double*)B.p, sB, (double*)L.p, (double*)X.p));
  return NULL;
}
static napi_value js_zhegvals(napi_env env, napi_callback_info info) {
  ARGS(6, "zhegvals_batched");
  int64_t batch, N, sB; opnd A, B, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, A) || F64(3, B) || get_i64(env, a[4], &sB) || F64(5, L)) return NULL;
  NEED(ZHEGV_FITS(N), "zhegvals_batched: buffer too small");
  SAME_SIDE(A.dev == B.dev && B.dev == L.dev, "zhegvals_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zhegvd[A.dev](g_handle, batch, N, (const double*)A.p, (const double*)B.p, sB, (double*)L.p, NULL));
  return NULL;
}
static napi_value js_zhegvx(napi_env env, napi_callback_info info) {
  ARGS(9, "zhegvx_batched");
  int64_t batch, N, i0, i1, sB; opnd A, B, L, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &i0) || get_i64(env, a[3], &i1) || F64(4, A) || F64(5, B) ||
      get_i64(env, a[6], &sB) || F64(7, L) || F64(8, X)) return NULL;
  NEED(0 <= i0 && i0 <= i1 && i1 <= N && ZHEGV_FITS(i1 - i0) && (size_t)(2 * batch * N * (i1 - i0)) <= X.len,
       "zhegvx_batched: bad subset or buffer too small");
  SAME_SIDE(A.dev == B.dev && B.dev == L.dev && L.dev == X.dev, "zhegvx_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zhegvx[A.dev](g_handle, batch, N, i0, i1, (const double*)A.p, (const double*)B.p, sB, (double*)L.p, (double*)X.p));
  return NULL;
}
static napi_value js_zhegvxals(napi_env env, napi_callback_info info) {
  ARGS(8, "zhegvxals_batched");
  int64_t batch, N, i0, i1, sB; opnd A, B, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &i0) || get_i64(env, a[3], &i1) || F64(4, A) || F64(5, B) ||
      get_i64(env, a[6], &sB) || F64(7, L)) return NULL;
  NEED(0 <= i0 && i0 <= i1 && i1 <= N && ZHEGV_FITS(i1 - i0), "zhegvxals_batched: bad subset or buffer too small");
  SAME_SIDE(A.dev == B.dev && B.dev == L.dev, "zhegvxals_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zhegvx[A.dev](g_handle, batch, N, i0, i1, (const double*)A.p, (const double*)B.p, sB, (double*)L.p, NULL));
  return NULL;
}
/* dsygvd_batched(algo, batch, N, A, B, strideB, L, X) / dsygvals_batched(algo, batch, N, A, B, strideB, L)   (eigen_sym_gen /
 * eigenvals_sym_gen: A x = lambda B x; algo 0 dc, 1 jacobi; strideB N*N or 0 = one B; the sweep counts are not asked for) */
static napi_value js_dsygvd(napi_env env, napi_callback_info info) {
  ARGS(8, "dsygvd_batched");
  int64_t algo, batch, N, sB; opnd A, B, L, X;
  if (get_i64(env, a[0], &algo) || get_i64(env, a[1], &batch) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, B) || get_i64(env, a[5], &sB) ||
      F64(6, L) || F64(7, X)) return NULL;
  NEED(batch >= 0 && N >= 0 && (sB == 0 || sB == N * N) && (size_t)(batch * N * N) <= A.len && (size_t)((sB ? batch : 1) * N * N) <= B.len &&
       (size_t)(batch * N) <= L.len && (size_t)(batch * N * N) <= X.len, "dsygvd_batched: buffer too small");
  SAME_SIDE(A.dev == B.dev && B.dev == L.dev && L.dev == X.dev, "dsygvd_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsygvd[A.dev](g_handle, (int)algo, batch, N, (const double*)A.p, (const double*)B.p, sB, (double*)L.p, (double*)X.p, NULL));
  return NULL;
}
static napi_value js_dsygvals(napi_env env, napi_callback_info info) {
  ARGS(7, "dsygvals_batched");
  int64_t algo, batch, N, sB; opnd A, B, L;
  if (get_i64(env, a[0], &algo) || get_i64(env, a[1], &batch) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, B) || get_i64(env, a[5], &sB) ||
      F64(6, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (sB == 0 || sB == N * N) && (size_t)(batch * N * N) <= A.len && (size_t)((sB ? batch : 1) * N * N) <= B.len &&
       (size_t)(batch * N) <= L.len, "dsygvals_batched: buffer too small");
  SAME_SIDE(A.dev == B.dev && B.dev == L.dev, "dsygvals_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsygvd[A.dev](g_handle, (int)algo, batch, N, (const double*)A.p, (const double*)B.p, sB, (double*)L.p, NULL, NULL));
  return NULL;
}
/* ---- the tridiagonal solver and the interval forms (csrc/syevx.hip). An operand that the call does not
 * need is passed as null: e for N = 1, Z / V / X for the values alone, bounds and range where no interval is selected. The interval
 * forms return kmax as a number. ---- */
static int is_nullish(napi_env env, napi_value v) {
  napi_valuetype t;
  return napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined);
}
/* an optional operand: absent -> p = NULL, and it takes the side of the others */
static int opt_op(napi_env env, napi_value v, napi_typedarray_type want, int side, opnd* out) {
  if (is_nullish(env, v)) { out->p = NULL; out->len = 0; out->dev = side; return 0; }
  return get_op(env, v, want, out);
}
static napi_value kmax_value(napi_env env, int64_t kmax) { napi_value r; napi_create_double(env, (double)kmax, &r); return r; }
/* dstcnt_batched(batch, N, M, d, e, x, count) */
static napi_value js_dstcnt(napi_env env, napi_callback_info info) {
  ARGS(7, "dstcnt_batched");
  int64_t batch, N, M; opnd d, e, x, c;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &M) || F64(3, d) || opt_op(env, a[4], napi_float64_array, d.dev, &e) ||
      F64(5, x) || I32(6, c)) return NULL;
  NEED(batch >= 0 && N >= 1 && M >= 0 && (size_t)(batch * N) <= d.len && (N < 2 || (size_t)(batch * (N - 1)) <= e.len) && (size_t)(batch * M) <= x.len &&
       (size_t)(batch * M) <= c.len, "dstcnt_batched: buffer too small");
  SAME_SIDE(d.dev == e.dev && e.dev == x.dev && x.dev == c.dev, "dstcnt_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dstcnt[d.dev](g_handle, batch, N, M, (const double*)d.p, (const double*)e.p, (const double*)x.p, (int32_t*)c.p));
  return NULL;
}
/* dstevx_batched(batch, N, i0, i1, d, e, L, Z): L [batch, k], Z [batch, k, N] (rows = vectors) or null */
static napi_value js_dstevx(napi_env env, napi_callback_info info) {
  ARGS(8, "dstevx_batched");
  int64_t batch, N, i0, i1; opnd d, e, L, Z;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &i0) || get_i64(env, a[3], &i1) || F64(4, d) ||
      opt_op(env, a[5], napi_float64_array, d.dev, &e) || F64(6, L) || opt_op(env, a[7], napi_float64_array, d.dev, &Z)) return NULL;
  NEED(batch >= 0 && N >= 1 && 0 <= i0 && i0 <= i1 && i1 <= N && (size_t)(batch * N) <= d.len && (N < 2 || (size_t)(batch * (N - 1)) <= e.len) &&
       (size_t)(batch * (i1 - i0)) <= L.len && (!Z.p || (size_t)(batch * (i1 - i0) * N) <= Z.len), "dstevx_batched: bad subset or buffer too small");
  SAME_SIDE(d.dev == e.dev && e.dev == L.dev && L.dev == Z.dev, "dstevx_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dstevx[d.dev](g_handle, batch, N, i0, i1, (const double*)d.p, (const double*)e.p, (double*)L.p, (double*)Z.p));
  return NULL;
}
/* dbdsvdx_batched(batch, K, J, i0, i1, d, e, U2, sv, V2, fallback): U2 [batch, K, k] and V2 [batch, k, J] or both null; fallback int32 [batch] or null */
static napi_value js_dbdsvdx(napi_env env, napi_callback_info info) {
  ARGS(11, "dbdsvdx_batched");
  int64_t batch, K, J, i0, i1; opnd d, e, U, S, V, fb;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &K) || get_i64(env, a[2], &J) || get_i64(env, a[3], &i0) || get_i64(env, a[4], &i1) ||
      F64(5, d) || opt_op(env, a[6], napi_float64_array, d.dev, &e) || opt_op(env, a[7], napi_float64_array, d.dev, &U) || F64(8, S) ||
      opt_op(env, a[9], napi_float64_array, d.dev, &V) || opt_op(env, a[10], napi_int32_array, d.dev, &fb)) return NULL;
  NEED(batch >= 0 && K >= 1 && (J == K || J == K + 1) && 0 <= i0 && i0 <= i1 && i1 <= K && (size_t)(batch * K) <= d.len &&
       (J < 2 || (size_t)(batch * (J - 1)) <= e.len) && (size_t)(batch * (i1 - i0)) <= S.len && !U.p == !V.p &&
       (!U.p || ((size_t)(batch * K * (i1 - i0)) <= U.len && (size_t)(batch * (i1 - i0) * J) <= V.len)) && (!fb.p || (size_t)batch <= fb.len),
       "dbdsvdx_batched: bad subset or buffer too small");
  SAME_SIDE(d.dev == e.dev && e.dev == U.dev && U.dev == S.dev && S.dev == V.dev && V.dev == fb.dev, "dbdsvdx_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dbdsvdx[d.dev](g_handle, batch, K, J, i0, i1, (const double*)d.p, (const double*)e.p, (double*)U.p, (double*)S.p, (double*)V.p,
                           (int32_t*)fb.p));
  return NULL;
}
/* dgesvdx_batched(batch, M, N, i0, i1, A, U, sv, V, fallback): U [batch, M, k] and V [batch, k, N] or both null; fallback int32 [batch] or null */
static napi_value js_dgesvdx(napi_env env, napi_callback_info info) {
  ARGS(10, "dgesvdx_batched");
  int64_t batch, M, N, i0, i1; opnd A, U, S, V, fb;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || get_i64(env, a[3], &i0) || get_i64(env, a[4], &i1) ||
      F64(5, A) || opt_op(env, a[6], napi_float64_array, A.dev, &U) || F64(7, S) || opt_op(env, a[8], napi_float64_array, A.dev, &V) ||
      opt_op(env, a[9], napi_int32_array, A.dev, &fb)) return NULL;
  NEED(batch >= 0 && M >= 1 && N >= 1 && 0 <= i0 && i0 <= i1 && i1 <= (M < N ? M : N) && (size_t)(batch * M * N) <= A.len &&
       (size_t)(batch * (i1 - i0)) <= S.len && !U.p == !V.p &&
       (!U.p || ((size_t)(batch * M * (i1 - i0)) <= U.len && (size_t)(batch * (i1 - i0) * N) <= V.len)) && (!fb.p || (size_t)batch <= fb.len),
       "dgesvdx_batched: bad subset or buffer too small");
  SAME_SIDE(A.dev == U.dev && U.dev == S.dev && S.dev == V.dev && V.dev == fb.dev, "dgesvdx_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dgesvdx[A.dev](g_handle, batch, M, N, i0, i1, (const double*)A.p, (double*)U.p, (double*)S.p, (double*)V.p, (int32_t*)fb.p));
  return NULL;
}
/* dstevxv_batched(batch, N, kcap, bounds, d, e, L, Z, range) -> kmax: L [batch, kcap], Z [batch, kcap, N] or null, range int32 [batch, 2] */
static napi_value js_dstevxv(napi_env env, napi_callback_info info) {
  ARGS(9, "dstevxv_batched");
  int64_t batch, N, kcap, kmax = 0; opnd bd, d, e, L, Z, rg;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &kcap) || F64(3, bd) || F64(4, d) ||
      opt_op(env, a[5], napi_float64_array, d.dev, &e) || F64(6, L) || opt_op(env, a[7], napi_float64_array, d.dev, &Z) || I32(8, rg)) return NULL;
  NEED(batch >= 0 && N >= 1 && kcap >= 0 && (size_t)(batch * 2) <= bd.len && (size_t)(batch * N) <= d.len && (N < 2 || (size_t)(batch * (N - 1)) <= e.len) &&
       (size_t)(batch * kcap) <= L.len && (!Z.p || (size_t)(batch * kcap * N) <= Z.len) && (size_t)(batch * 2) <= rg.len, "dstevxv_batched: buffer too small");
  SAME_SIDE(bd.dev == d.dev && d.dev == e.dev && e.dev == L.dev && L.dev == Z.dev && Z.dev == rg.dev, "dstevxv_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dstevxv[d.dev](g_handle, batch, N, kcap, (const double*)bd.p, (const double*)d.p, (const double*)e.p, (double*)L.p, (double*)Z.p,
                           (int32_t*)rg.p, &kmax));
  return kmax_value(env, kmax);
}
/* dsyevxv_batched(tridiag, batch, N, kcap, bounds, S, L, V, range) -> kmax: L [batch, kcap], V [batch, N, kcap] or null */
static napi_value js_dsyevxv(napi_env env, napi_callback_info info) {
  ARGS(9, "dsyevxv_batched");
  int64_t tr, batch, N, kcap, kmax = 0; opnd bd, S, L, V, rg;
  if (get_i64(env, a[0], &tr) || get_i64(env, a[1], &batch) || get_i64(env, a[2], &N) || get_i64(env, a[3], &kcap) || F64(4, bd) || F64(5, S) ||
      F64(6, L) || opt_op(env, a[7], napi_float64_array, S.dev, &V) || I32(8, rg)) return NULL;
  NEED((tr == 0 || tr == 1) && batch >= 0 && N >= 0 && kcap >= 0 && (size_t)(batch * 2) <= bd.len && (size_t)(batch * N * N) <= S.len &&
       (size_t)(batch * kcap) <= L.len && (!V.p || (size_t)(batch * N * kcap) <= V.len) && (size_t)(batch * 2) <= rg.len, "dsyevxv_batched: buffer too small");
  SAME_SIDE(bd.dev == S.dev && S.dev == L.dev && L.dev == V.dev && V.dev == rg.dev, "dsyevxv_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsyevxv[tr][S.dev](g_handle, batch, N, kcap, (const double*)bd.p, (const double*)S.p, (double*)L.p, (double*)V.p, (int32_t*)rg.p, &kmax));
  return kmax_value(env, kmax);
}
/* dsygvx_batched(reduction, select, batch, N, i0, i1, kcap, bounds, A, B, strideB, L, X, range) -> kmax (0 unless select = 2): L and X are
 * K = N (select 0), i1 - i0 (1) or kcap (2) wide; bounds and range are null unless select = 2; X null: the values alone */
static napi_value js_dsygvx(napi_env env, napi_callback_info info) {
  ARGS(14, "dsygvx_batched");
  int64_t red, sel, batch, N, i0, i1, kcap, sB, kmax = 0; opnd bd, A, B, L, X, rg;
  if (get_i64(env, a[0], &red) || get_i64(env, a[1], &sel) || get_i64(env, a[2], &batch) || get_i64(env, a[3], &N) || get_i64(env, a[4], &i0) ||
      get_i64(env, a[5], &i1) || get_i64(env, a[6], &kcap) || F64(8, A) || opt_op(env, a[7], napi_float64_array, A.dev, &bd) || F64(9, B) ||
      get_i64(env, a[10], &sB) || F64(11, L) || opt_op(env, a[12], napi_float64_array, A.dev, &X) || opt_op(env, a[13], napi_int32_array, A.dev, &rg)) return NULL;
  NEED(sel >= 0 && sel <= 2 && batch >= 0 && N >= 0 && (sel != 1 || (0 <= i0 && i0 <= i1 && i1 <= N)) && (sel != 2 || kcap >= 0), "dsygvx_batched: bad selector");
  const int64_t K = sel == 0 ? N : sel == 1 ? i1 - i0 : kcap;
  NEED((sB == 0 || sB == N * N) && (size_t)(batch * N * N) <= A.len && (size_t)((sB ? batch : 1) * N * N) <= B.len && (size_t)(batch * K) <= L.len &&
       (!X.p || (size_t)(batch * N * K) <= X.len) && (sel != 2 || (bd.p && rg.p && (size_t)(batch * 2) <= bd.len && (size_t)(batch * 2) <= rg.len)),
       "dsygvx_batched: buffer too small");
  SAME_SIDE(A.dev == B.dev && B.dev == L.dev && L.dev == X.dev && X.dev == bd.dev && bd.dev == rg.dev, "dsygvx_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsygvx[A.dev](g_handle, (int)red, (int)sel, batch, N, i0, i1, kcap, (const double*)bd.p, (const double*)A.p, (const double*)B.p, sB,
                          (double*)L.p, (double*)X.p, (int32_t*)rg.p, sel == 2 ? &kmax : NULL));
  return kmax_value(env, kmax);
}
/* dnrmfro(n, A) -> number   (norm(A) 'fro', norm.js:22-85); a device operand's result comes back as a host number too */
static napi_value js_dnrmfro(napi_env env, napi_callback_info info) {
  ARGS(2, "dnrmfro");
  int64_t n; opnd A;
  if (get_i64(env, a[0], &n) || F64(1, A)) return NULL;
  NEED(n >= 0 && (size_t)n <= A.len, "dnrmfro: buffer too small");
  if (ensure_handle(env)) return NULL;
  double out = 0.0;
  if (!A.dev || n == 0) {
    FAIL_IF(p_dnrmfro[0](g_handle, n, A.dev ? NULL : (const double*)A.p, &out));
  } else {
    void* d = NULL;
    FAIL_IF(p_malloc(g_handle, sizeof(double), &d));
    int rc = p_dnrmfro[1](g_handle, n, (const double*)A.p, (double*)d);
    if (rc == 0) rc = p_d2h(g_handle, &out, d, sizeof(double));
    p_free(g_handle, d);
    FAIL_IF(rc);
  }
  napi_value r;
  napi_create_double(env, out, &r);
  return r;
}
/* dqp3rank_batched(batch, M, N, R, rank)   (rrqr_rank, rrqr.js:398-414; host form throws the reference's message) */
static napi_value js_dqp3rank(napi_env env, napi_callback_info info) {
  ARGS(5, "dqp3rank_batched");
  int64_t batch, M, N; opnd R, r;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, R) || I32(4, r)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= R.len && (size_t)batch <= r.len, "dqp3rank_batched: buffer too small");
  SAME_SIDE(R.dev == r.dev, "dqp3rank_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dqp3rank[R.dev](g_handle, batch, M, N, (const double*)R.p, (int32_t*)r.p));
  return NULL;
}
/* dqp3ls_batched(batch, N, M, I, J, Q, strideQ, R, strideR, P, strideP, Y, strideY, X, rank)   (rrqr_lstsq, rrqr.js:447-580) */
static napi_value js_dqp3ls(napi_env env, napi_callback_info info) {
  ARGS(15, "dqp3ls_batched");
  int64_t batch, N, M, I, J, sQ, sR, sP, sY; opnd Q, R, P, Y, X, r;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &M) || get_i64(env, a[3], &I) || get_i64(env, a[4], &J) ||
      F64(5, Q) || get_i64(env, a[6], &sQ) || F64(7, R) || get_i64(env, a[8], &sR) || I32(9, P) || get_i64(env, a[10], &sP) ||
      F64(11, Y) || get_i64(env, a[12], &sY) || F64(13, X) || I32(14, r)) return NULL;
  NEED(batch >= 0 && N >= 0 && M >= 0 && I >= 0 && J >= 0 && sQ >= 0 && sR >= 0 && sP >= 0 && sY >= 0, "dqp3ls_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sQ + N * M) <= Q.len && (size_t)((batch - 1) * sR + M * I) <= R.len &&
                      (size_t)((batch - 1) * sP + I) <= P.len && (size_t)((batch - 1) * sY + N * J) <= Y.len &&
                      (size_t)(batch * I * J) <= X.len && (size_t)batch <= r.len), "dqp3ls_batched: buffer too small");
  SAME_SIDE(Q.dev == R.dev && R.dev == P.dev && P.dev == Y.dev && Y.dev == X.dev && X.dev == r.dev, "dqp3ls_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dqp3ls[X.dev](g_handle, batch, N, M, I, J, (const double*)Q.p, sQ, (const double*)R.p, sR, (const int32_t*)P.p, sP,
                          (const double*)Y.p, sY, (double*)X.p, (int32_t*)r.p));
  return NULL;
}
/* dsvdls_batched(batch, N, M, I, J, U, strideU, sv, strideSv, V, strideV, Y, strideY, X)   (svd_lstsq, svd.js:100-228) */
static napi_value js_dsvdls(napi_env env, napi_callback_info info) {
  ARGS(14, "dsvdls_batched");
  int64_t batch, N, M, I, J, sU, sS, sV, sY; opnd U, S, V, Y, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &M) || get_i64(env, a[3], &I) || get_i64(env, a[4], &J) ||
      F64(5, U) || get_i64(env, a[6], &sU) || F64(7, S) || get_i64(env, a[8], &sS) || F64(9, V) || get_i64(env, a[10], &sV) ||
      F64(11, Y) || get_i64(env, a[12], &sY) || F64(13, X)) return NULL;
  NEED(batch >= 0 && N >= 0 && M >= 0 && I >= 0 && J >= 0 && sU >= 0 && sS >= 0 && sV >= 0 && sY >= 0, "dsvdls_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sU + N * M) <= U.len && (size_t)((batch - 1) * sS + M) <= S.len &&
                      (size_t)((batch - 1) * sV + M * I) <= V.len && (size_t)((batch - 1) * sY + N * J) <= Y.len && (size_t)(batch * I * J) <= X.len),
       "dsvdls_batched: buffer too small");
  SAME_SIDE(U.dev == S.dev && S.dev == V.dev && V.dev == Y.dev && Y.dev == X.dev, "dsvdls_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsvdls[X.dev](g_handle, batch, N, M, I, J, (const double*)U.p, sU, (const double*)S.p, sS, (const double*)V.p, sV,
                          (const double*)Y.p, sY, (double*)X.p));
  return NULL;
}

/* dpotrf_batched(batch, N, S, L)   (cholesky_decomp, cholesky.js:51-71) */
static napi_value js_dpotrf(napi_env env, napi_callback_info info) {
  ARGS(4, "dpotrf_batched");
  int64_t batch, N; opnd S, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, S) || F64(3, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= S.len && (size_t)(batch * N * N) <= L.len, "dpotrf_batched: buffer too small");
  SAME_SIDE(S.dev == L.dev, "dpotrf_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dpotrf[S.dev](g_handle, batch, N, (const double*)S.p, (double*)L.p));
  return NULL;
}
/* dpotrs_batched(batch, N, J, L, strideL, Y, strideY, X)   (cholesky_solve, cholesky.js:74-150) */
static napi_value js_dpotrs(napi_env env, napi_callback_info info) {
  ARGS(8, "dpotrs_batched");
  int64_t batch, N, J, sL, sY; opnd L, Y, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &J) || F64(3, L) || get_i64(env, a[4], &sL) ||
      F64(5, Y) || get_i64(env, a[6], &sY) || F64(7, X)) return NULL;
  NEED(batch >= 0 && N >= 0 && J >= 0 && sL >= 0 && sY >= 0, "dpotrs_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sL + N * N) <= L.len && (size_t)((batch - 1) * sY + N * J) <= Y.len && (size_t)(batch * N * J) <= X.len),
       "dpotrs_batched: buffer too small");
  SAME_SIDE(L.dev == Y.dev && Y.dev == X.dev, "dpotrs_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dpotrs[X.dev](g_handle, batch, N, J, (const double*)L.p, sL, (const double*)Y.p, sY, (double*)X.p));
  return NULL;
}

/* dldltrf_batched(batch, N, S, LD)   (ldl_decomp, ldl.js:67-90) */
static napi_value js_dldltrf(napi_env env, napi_callback_info info) {
  ARGS(4, "dldltrf_batched");
  int64_t batch, N; opnd S, L;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, S) || F64(3, L)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= S.len && (size_t)(batch * N * N) <= L.len, "dldltrf_batched: buffer too small");
  SAME_SIDE(S.dev == L.dev, "dldltrf_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dldltrf[S.dev](g_handle, batch, N, (const double*)S.p, (double*)L.p));
  return NULL;
}
/* dsytrf_bk_batched(batch, N, S, LD, P, tier)   (pldlp_decomp, pldlp.js:191-222; tier: ND4HIP_PLDLP_TIER_*) */
static napi_value js_dsytrf_bk(napi_env env, napi_callback_info info) {
  ARGS(6, "dsytrf_bk_batched");
  int64_t batch, N, tier; opnd S, L, P;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, S) || F64(3, L) || I32(4, P) || get_i64(env, a[5], &tier)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N * N) <= S.len && (size_t)(batch * N * N) <= L.len && (size_t)(batch * N) <= P.len,
       "dsytrf_bk_batched: buffer too small");
  SAME_SIDE(S.dev == L.dev && L.dev == P.dev, "dsytrf_bk_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsytrf_bk[S.dev](g_handle, batch, N, (const double*)S.p, (double*)L.p, (int32_t*)P.p, (int)tier));
  return NULL;
}
/* dsytrs_bk_batched(batch, N, J, LD, strideLD, P, strideP, Y, strideY, X)   (pldlp_solve, pldlp.js:519-604) */
static napi_value js_dsytrs_bk(napi_env env, napi_callback_info info) {
  ARGS(10, "dsytrs_bk_batched");
  int64_t batch, N, J, sL, sP, sY; opnd L, P, Y, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &J) || F64(3, L) || get_i64(env, a[4], &sL) ||
      I32(5, P) || get_i64(env, a[6], &sP) || F64(7, Y) || get_i64(env, a[8], &sY) || F64(9, X)) return NULL;
  NEED(batch >= 0 && N >= 0 && J >= 0 && sL >= 0 && sP >= 0 && sY >= 0, "dsytrs_bk_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sL + N * N) <= L.len && (size_t)((batch - 1) * sP + N) <= P.len &&
                      (size_t)((batch - 1) * sY + N * J) <= Y.len && (size_t)(batch * N * J) <= X.len), "dsytrs_bk_batched: buffer too small");
  SAME_SIDE(L.dev == P.dev && P.dev == Y.dev && Y.dev == X.dev, "dsytrs_bk_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dsytrs_bk[X.dev](g_handle, batch, N, J, (const double*)L.p, sL, (const int32_t*)P.p, sP, (const double*)Y.p, sY, (double*)X.p));
  return NULL;
}
/* structure functions (tri.js:23-42, diag.js:23-88, permute.js:23-306, NDArray.T): values are moved, never computed
 * dtranspose_batched(batch, M, N, A, B)   B [batch,N,M] */
static napi_value js_dtranspose(napi_env env, napi_callback_info info) {
  ARGS(5, "dtranspose_batched");
  int64_t batch, M, N; opnd A, B;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || F64(3, A) || F64(4, B)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * N) <= B.len, "dtranspose_batched: buffer too small");
  SAME_SIDE(A.dev == B.dev, "dtranspose_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dtranspose[A.dev](g_handle, batch, M, N, (const double*)A.p, (double*)B.p));
  return NULL;
}
/* dtri_batched(upper, k, batch, M, N, A, B)   tril (upper = 0) / triu */
static napi_value js_dtri(napi_env env, napi_callback_info info) {
  ARGS(7, "dtri_batched");
  int64_t upper, k, batch, M, N; opnd A, B;
  if (get_i64(env, a[0], &upper) || get_i64(env, a[1], &k) || get_i64(env, a[2], &batch) || get_i64(env, a[3], &M) || get_i64(env, a[4], &N) ||
      F64(5, A) || F64(6, B)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && (size_t)(batch * M * N) <= A.len && (size_t)(batch * M * N) <= B.len, "dtri_batched: buffer too small");
  SAME_SIDE(A.dev == B.dev, "dtri_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dtri[A.dev](g_handle, upper != 0, k, batch, M, N, (const double*)A.p, (double*)B.p));
  return NULL;
}
/* ddiag_batched(batch, M, N, offset, A, d)   d [batch, min(M, M+offset, N, N-offset)] */
static napi_value js_ddiag(napi_env env, napi_callback_info info) {
  ARGS(6, "ddiag_batched");
  int64_t batch, M, N, off; opnd A, d;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &M) || get_i64(env, a[2], &N) || get_i64(env, a[3], &off) || F64(4, A) || F64(5, d)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && off > -M && off < N, "ddiag_batched: bad extent or offset");
  {
    int64_t L = M < N ? M : N;
    if (M + off < L) L = M + off;
    if (N - off < L) L = N - off;
    NEED((size_t)(batch * M * N) <= A.len && (size_t)(batch * L) <= d.len, "ddiag_batched: buffer too small");
  }
  SAME_SIDE(A.dev == d.dev, "ddiag_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_ddiag[A.dev](g_handle, batch, M, N, off, (const double*)A.p, (double*)d.p));
  return NULL;
}
/* ddiagmat_batched(batch, N, d, D)   D [batch,N,N] */
static napi_value js_ddiagmat(napi_env env, napi_callback_info info) {
  ARGS(4, "ddiagmat_batched");
  int64_t batch, N; opnd d, D;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || F64(2, d) || F64(3, D)) return NULL;
  NEED(batch >= 0 && N >= 0 && (size_t)(batch * N) <= d.len && (size_t)(batch * N * N) <= D.len, "ddiagmat_batched: buffer too small");
  SAME_SIDE(d.dev == D.dev, "ddiagmat_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_ddiagmat[d.dev](g_handle, batch, N, (const double*)d.p, (double*)D.p));
  return NULL;
}
/* dpermute_batched(cols, inverse, batch, M, N, A, strideA, P, strideP, B)   permute_rows / _cols, unpermute_rows / _cols */
static napi_value js_dpermute(napi_env env, napi_callback_info info) {
  ARGS(10, "dpermute_batched");
  int64_t cols, inverse, batch, M, N, sA, sP; opnd A, P, B;
  if (get_i64(env, a[0], &cols) || get_i64(env, a[1], &inverse) || get_i64(env, a[2], &batch) || get_i64(env, a[3], &M) || get_i64(env, a[4], &N) ||
      F64(5, A) || get_i64(env, a[6], &sA) || I32(7, P) || get_i64(env, a[8], &sP) || F64(9, B)) return NULL;
  NEED(batch >= 0 && M >= 0 && N >= 0 && sA >= 0 && sP >= 0, "dpermute_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sA + M * N) <= A.len && (size_t)((batch - 1) * sP + (cols ? N : M)) <= P.len &&
                      (size_t)(batch * M * N) <= B.len), "dpermute_batched: buffer too small");
  SAME_SIDE(A.dev == P.dev && P.dev == B.dev, "dpermute_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dpermute[A.dev](g_handle, cols != 0, inverse != 0, batch, M, N, (const double*)A.p, sA, (const int32_t*)P.p, sP, (double*)B.p));
  return NULL;
}
/* up to 8 numbers of a JS array */
static int get_i64_list(napi_env env, napi_value v, int64_t* out, uint32_t* n) {
  bool is_arr = false;
  napi_is_array(env, v, &is_arr);
  if (!is_arr || napi_get_array_length(env, v, n) != napi_ok) { napi_throw_type_error(env, "ND4HIP", "expected an array of numbers"); return -1; }
  if (*n > 8) { napi_throw_range_error(env, "ND4HIP", "gather_nd: more than 8 axes"); return -1; }
  for (uint32_t i = 0; i < *n; i++) {
    napi_value e;
    if (napi_get_element(env, v, i, &e) != napi_ok || get_i64(env, e, &out[i])) return -1;
  }
  return 0;
}
/* gather_nd(elemBytes, shape, src, srcOff, srcStrides, dst, dstOff, dstStrides): the strided N-d copy of sliceElems, transpose(...axes),
 * concat and stack; src and dst are device views, their lengths are what the library checks the box against. Device only. */
static napi_value js_gather_nd(napi_env env, napi_callback_info info) {
  ARGS(8, "gather_nd");
  int64_t eb, so, dof, shape[8], ss[8], ds[8]; uint32_t nd = 0, ns = 0, nt = 0; opnd S, D;
  if (get_i64(env, a[0], &eb) || get_i64_list(env, a[1], shape, &nd) || get_i64(env, a[3], &so) || get_i64_list(env, a[4], ss, &ns) ||
      get_i64(env, a[6], &dof) || get_i64_list(env, a[7], ds, &nt)) return NULL;
  NEED(eb == 4 || eb == 8, "gather_nd: elemBytes must be 4 or 8");
  NEED(ns == nd && nt == nd, "gather_nd: shape and strides must have one length");
  if (get_op(env, a[2], eb == 8 ? napi_float64_array : napi_int32_array, &S) || get_op(env, a[5], eb == 8 ? napi_float64_array : napi_int32_array, &D)) return NULL;
  if (!(S.dev == 1 && D.dev == 1)) { napi_throw_type_error(env, "ND4HIP", "gather_nd: device views only (there is no host-pointer form)"); return NULL; }
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_gather_nd(g_handle, (int)eb, (int)nd, shape, S.p, (int64_t)S.len, so, ss, D.p, (int64_t)D.len, dof, ds));
  return NULL;
}
/* zip_nd(op, shape, A, aOff, aStrides, B | null, bOff, bStrides, C): C[i] = op(A[..], B[..]) on float64 device views (zip_elems and
 * mapElems with one of nd.math's operators); C is dense, with one element per index of the box. Device only. */
static napi_value js_zip_nd(napi_env env, napi_callback_info info) {
  ARGS(9, "zip_nd");
  int64_t op, ao, bo = 0, shape[8], as[8], bs[8]; uint32_t nd = 0, na = 0, nb = 0; opnd A, B, C;
  napi_valuetype tb;
  if (get_i64(env, a[0], &op) || get_i64_list(env, a[1], shape, &nd) || get_i64(env, a[3], &ao) || get_i64_list(env, a[4], as, &na) ||
      napi_typeof(env, a[5], &tb) != napi_ok) return NULL;
  const int unary = tb == napi_null || tb == napi_undefined;
  NEED(na == nd, "zip_nd: shape and strides must have one length");
  if (F64(2, A) || F64(8, C)) return NULL;
  B.p = NULL; B.len = 0; B.dev = 1;
  if (!unary) {
    if (get_i64(env, a[6], &bo) || get_i64_list(env, a[7], bs, &nb) || F64(5, B)) return NULL;
    NEED(nb == nd, "zip_nd: shape and strides must have one length");
  }
  if (!(A.dev == 1 && B.dev == 1 && C.dev == 1)) { napi_throw_type_error(env, "ND4HIP", "zip_nd: device views only (there is no host-pointer form)"); return NULL; }
  int64_t count = 1;
  for (uint32_t i = 0; i < nd; i++) { NEED(shape[i] >= 1 && count <= INT64_MAX / shape[i], "zip_nd: bad extent"); count *= shape[i]; }
  NEED((size_t)count <= C.len, "zip_nd: C is too small");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_zip_nd(g_handle, (int)op, (int)nd, shape, (const double*)A.p, (int64_t)A.len, ao, as, (const double*)B.p, (int64_t)B.len, bo, bs,
                   (double*)C.p, count));
  return NULL;
}
/* reduce_nd(op, shape, reduced, A, C): reduceElems with add, mul, min or max in the reference's order; reduced[d] != 0 folds axis d
 * away. A and C are device views that start at the operand and at the result. Device only. */
static napi_value js_reduce_nd(napi_env env, napi_callback_info info) {
  ARGS(5, "reduce_nd");
  int64_t op, shape[8], red[8]; int32_t flags[8]; uint32_t nd = 0, nr = 0; opnd A, C;
  if (get_i64(env, a[0], &op) || get_i64_list(env, a[1], shape, &nd) || get_i64_list(env, a[2], red, &nr) || F64(3, A) || F64(4, C)) return NULL;
  NEED(nr == nd, "reduce_nd: shape and flags must have one length");
  int64_t outs = 1;
  for (uint32_t i = 0; i < nd; i++) {
    NEED(shape[i] >= 1 && outs <= INT64_MAX / shape[i], "reduce_nd: bad extent");
    flags[i] = red[i] != 0;
    if (!flags[i]) outs *= shape[i];
  }
  NEED((size_t)outs <= C.len, "reduce_nd: C is too small");
  if (!(A.dev == 1 && C.dev == 1)) { napi_throw_type_error(env, "ND4HIP", "reduce_nd: device views only (there is no host-pointer form)"); return NULL; }
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_reduce_nd(g_handle, (int)op, (int)nd, shape, flags, (const double*)A.p, (int64_t)A.len, (double*)C.p, outs));
  return NULL;
}
/* dldltrs_batched(batch, N, J, LD, strideLD, Y, strideY, X)   (ldl_solve, ldl.js:133-201) */
static napi_value js_dldltrs(napi_env env, napi_callback_info info) {
  ARGS(8, "dldltrs_batched");
  int64_t batch, N, J, sL, sY; opnd L, Y, X;
  if (get_i64(env, a[0], &batch) || get_i64(env, a[1], &N) || get_i64(env, a[2], &J) || F64(3, L) || get_i64(env, a[4], &sL) ||
      F64(5, Y) || get_i64(env, a[6], &sY) || F64(7, X)) return NULL;
  NEED(batch >= 0 && N >= 0 && J >= 0 && sL >= 0 && sY >= 0, "dldltrs_batched: negative extent");
  NEED(batch == 0 || ((size_t)((batch - 1) * sL + N * N) <= L.len && (size_t)((batch - 1) * sY + N * J) <= Y.len && (size_t)(batch * N * J) <= X.len),
       "dldltrs_batched: buffer too small");
  SAME_SIDE(L.dev == Y.dev && Y.dev == X.dev, "dldltrs_batched");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_dldltrs[X.dev](g_handle, batch, N, J, (const double*)L.p, sL, (const double*)Y.p, sY, (double*)X.p));
  return NULL;
}

/* ---- device memory ---- */
/* dev_alloc(bytes) -> buffer */
static napi_value js_dev_alloc(napi_env env, napi_callback_info info) {
  ARGS(1, "dev_alloc");
  int64_t bytes;
  if (get_i64(env, a[0], &bytes)) return NULL;
  NEED(bytes >= 0, "dev_alloc: negative size");
  if (ensure_handle(env)) return NULL;
  devbuf* b = (devbuf*)calloc(1, sizeof(devbuf));
  if (!b) THROW(env, "dev_alloc: out of host memory");
  b->magic = DEVBUF_MAGIC; b->bytes = (size_t)bytes;
  if (p_malloc(g_handle, b->bytes, &b->p) != 0) { free(b); THROW(env, p_last_error()); }
  napi_value r;
  if (napi_create_external(env, b, devbuf_finalize, NULL, &r) != napi_ok) { devbuf_release(b); free(b); THROW(env, "dev_alloc: napi_create_external failed"); }
  int64_t adj; napi_adjust_external_memory(env, (int64_t)b->bytes, &adj);     /* let the GC see the device bytes it keeps alive */
  return r;
}
/* dev_free(buffer): idempotent; the finalizer covers buffers that are simply dropped */
static napi_value js_dev_free(napi_env env, napi_callback_info info) {
  ARGS(1, "dev_free");
  devbuf* b = get_devbuf(env, a[0]);
  if (!b) return NULL;
  if (b->p) { int64_t adj; napi_adjust_external_memory(env, -(int64_t)b->bytes, &adj); devbuf_release(b); b->bytes = 0; }
  return NULL;
}
static int get_any_ta(napi_env env, napi_value v, void** data, size_t* bytes) {
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  napi_typedarray_type type; napi_value buf; size_t off, len;
  if (!is_ta || napi_get_typedarray_info(env, v, &type, &len, data, &buf, &off) != napi_ok ||
      (type != napi_float64_array && type != napi_int32_array)) {
    napi_throw_type_error(env, "ND4HIP", "expected a Float64Array or an Int32Array");
    return -1;
  }
  *bytes = len * (type == napi_float64_array ? 8 : 4);
  return 0;
}
/* dev_upload(buffer, byteOffset, typedArray): blocking H2D */
static napi_value js_dev_upload(napi_env env, napi_callback_info info) {
  ARGS(3, "dev_upload");
  devbuf* b = get_devbuf(env, a[0]);
  int64_t off; void* src; size_t bytes;
  if (!b || get_i64(env, a[1], &off) || get_any_ta(env, a[2], &src, &bytes)) return NULL;
  NEED(b->p && off >= 0 && (size_t)off + bytes <= b->bytes, "dev_upload: out of range (or freed buffer)");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_h2d(g_handle, (char*)b->p + off, src, bytes));
  return NULL;
}
/* dev_download(typedArray, buffer, byteOffset): blocking D2H after everything queued on the handle's stream */
static napi_value js_dev_download(napi_env env, napi_callback_info info) {
  ARGS(3, "dev_download");
  devbuf* b = get_devbuf(env, a[1]);
  int64_t off; void* dst; size_t bytes;
  if (!b || get_i64(env, a[2], &off) || get_any_ta(env, a[0], &dst, &bytes)) return NULL;
  NEED(b->p && off >= 0 && (size_t)off + bytes <= b->bytes, "dev_download: out of range (or freed buffer)");
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_d2h(g_handle, dst, (const char*)b->p + off, bytes));
  return NULL;
}
static napi_value js_synchronize(napi_env env, napi_callback_info info) {
  (void)info;
  if (ensure_handle(env)) return NULL;
  FAIL_IF(p_sync(g_handle));
  return NULL;
}

static void cleanup(void* arg) {
  (void)arg;
  if (g_handle && p_destroy) { p_destroy(g_handle); g_handle = NULL; }
}

/* profile_enable(on) */
static napi_value js_profile_enable(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value a[1]; bool on = true;
  napi_get_cb_info(env, info, &argc, a, NULL, NULL);
  if (argc >= 1) napi_get_value_bool(env, a[0], &on);
  if (ensure_handle(env)) return NULL;
  if (p_prof_enable(g_handle, on ? 1 : 0) != 0) THROW(env, p_last_error());
  return NULL;
}
/* profile_last() -> [{device, valid, op, kernel_ms, flops, bytes}] : one record per device of the handle (nd4hip_profile_last) */
static napi_value js_profile_last(napi_env env, napi_callback_info info) {
  (void)info;
  if (ensure_handle(env)) return NULL;
  nd4hip_prof rec[64];
  const int n = p_prof_last(g_handle, rec, 64);
  if (n < 0) THROW(env, p_last_error());
  napi_value arr, o, v;
  napi_create_array_with_length(env, (size_t)n, &arr);
  for (int i = 0; i < n && i < 64; i++) {
    napi_create_object(env, &o);
    napi_create_int32(env, rec[i].device, &v); napi_set_named_property(env, o, "device", v);
    napi_get_boolean(env, rec[i].valid != 0, &v); napi_set_named_property(env, o, "valid", v);
    napi_create_string_utf8(env, rec[i].op, NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, o, "op", v);
    napi_create_double(env, rec[i].kernel_ms, &v); napi_set_named_property(env, o, "kernel_ms", v);
    napi_create_double(env, rec[i].flops, &v); napi_set_named_property(env, o, "flops", v);
    napi_create_double(env, rec[i].bytes, &v); napi_set_named_property(env, o, "bytes", v);
    napi_set_element(env, arr, (uint32_t)i, o);
  }
  return arr;
}

static napi_value init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
    {"device_count", NULL, js_device_count, NULL, NULL, NULL, napi_default, NULL},
    {"version", NULL, js_version, NULL, NULL, NULL, napi_default, NULL},
    {"devices", NULL, js_devices, NULL, NULL, NULL, napi_default, NULL},
    {"dgemm_batched", NULL, js_dgemm, NULL, NULL, NULL, napi_default, NULL},
    {"zgemm_batched", NULL, js_zgemm, NULL, NULL, NULL, napi_default, NULL},
    {"dgetrf_batched", NULL, js_dgetrf, NULL, NULL, NULL, napi_default, NULL},
    {"dgeqrf_q_batched", NULL, js_dgeqrf, NULL, NULL, NULL, napi_default, NULL},
    {"dgeqrf_full_batched", NULL, js_dgeqrf_full, NULL, NULL, NULL, napi_default, NULL},
    {"dgeqrf_qty_batched", NULL, js_dgeqrf_qty, NULL, NULL, NULL, napi_default, NULL},
    {"dgebrd_batched", NULL, js_dgebrd, NULL, NULL, NULL, napi_default, NULL},
    {"dgehrd_batched", NULL, js_dgehrd, NULL, NULL, NULL, napi_default, NULL},
    {"dgesvdj_batched", NULL, js_dgesvdj, NULL, NULL, NULL, napi_default, NULL},
    {"dgesdd_batched", NULL, js_dgesdd, NULL, NULL, NULL, napi_default, NULL},
    {"dgetrs_batched", NULL, js_dgetrs, NULL, NULL, NULL, napi_default, NULL},
    {"dqrls_batched", NULL, js_dqrls, NULL, NULL, NULL, napi_default, NULL},
    {"dsvdls_batched", NULL, js_dsvdls, NULL, NULL, NULL, napi_default, NULL},
    {"dgeqp3_batched", NULL, js_dgeqp3, NULL, NULL, NULL, napi_default, NULL},
    {"dgeqp3_full_batched", NULL, js_dgeqp3_full, NULL, NULL, NULL, napi_default, NULL},
    {"ddet_batched", NULL, js_ddet, NULL, NULL, NULL, napi_default, NULL},
    {"dslogdet_batched", NULL, js_dslogdet, NULL, NULL, NULL, napi_default, NULL},
    {"ddettri_batched", NULL, js_ddettri, NULL, NULL, NULL, napi_default, NULL},
    {"dslogdettri_batched", NULL, js_dslogdettri, NULL, NULL, NULL, napi_default, NULL},
    {"dnrmfro", NULL, js_dnrmfro, NULL, NULL, NULL, napi_default, NULL},
    {"dtreval_batched", NULL, js_dtreval, NULL, NULL, NULL, napi_default, NULL},
    {"dtrevc_batched", NULL, js_dtrevc, NULL, NULL, NULL, napi_default, NULL},
    {"dgebal_batched", NULL, js_dgebal, NULL, NULL, NULL, napi_default, NULL},
    {"zgebak_batched", NULL, js_zgebak, NULL, NULL, NULL, napi_default, NULL},
    {"dhseqr_batched", NULL, js_dhseqr, NULL, NULL, NULL, napi_default, NULL},
    {"dgees_batched", NULL, js_dgees, NULL, NULL, NULL, napi_default, NULL},
    {"dgeev_batched", NULL, js_dgeev, NULL, NULL, NULL, napi_default, NULL},
    {"dgeevals_batched", NULL, js_dgeevals, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevd_batched", NULL, js_dsyevd, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevals_batched", NULL, js_dsyevals, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevj_batched", NULL, js_dsyevj, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevjals_batched", NULL, js_dsyevjals, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevx_batched", NULL, js_dsyevx, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevxals_batched", NULL, js_dsyevxals, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevd_tr_batched", NULL, js_dsyevd_tr, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevdals_tr_batched", NULL, js_dsyevdals_tr, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevx_tr_batched", NULL, js_dsyevx_tr, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevxals_tr_batched", NULL, js_dsyevxals_tr, NULL, NULL, NULL, napi_default, NULL},
    {"zheevd_batched", NULL, js_zheevd, NULL, NULL, NULL, napi_default, NULL},
    {"zheevdals_batched", NULL, js_zheevdals, NULL, NULL, NULL, napi_default, NULL},
    {"zheevx_batched", NULL, js_zheevx, NULL, NULL, NULL, napi_default, NULL},
    {"zheevxals_batched", NULL, js_zheevxals, NULL, NULL, NULL, napi_default, NULL},
    {"zpotrf_batched", NULL, js_zpotrf, NULL, NULL, NULL, napi_default, NULL},
    {"zpotrs_batched", NULL, js_zpotrs, NULL, NULL, NULL, napi_default, NULL},
    {"zhegvd_batched", NULL, js_zhegvd, NULL, NULL, NULL, napi_default, NULL},
    {"zhegvals_batched", NULL, js_zhegvals, NULL, NULL, NULL, napi_default, NULL},
    {"zhegvx_batched", NULL, js_zhegvx, NULL, NULL, NULL, napi_default, NULL},
    {"zhegvxals_batched", NULL, js_zhegvxals, NULL, NULL, NULL, napi_default, NULL},
    {"dsygvd_batched", NULL, js_dsygvd, NULL, NULL, NULL, napi_default, NULL},
    {"dsygvals_batched", NULL, js_dsygvals, NULL, NULL, NULL, napi_default, NULL},
    {"dstcnt_batched", NULL, js_dstcnt, NULL, NULL, NULL, napi_default, NULL},
    {"dstevx_batched", NULL, js_dstevx, NULL, NULL, NULL, napi_default, NULL},
    {"dstevxv_batched", NULL, js_dstevxv, NULL, NULL, NULL, napi_default, NULL},
    {"dbdsvdx_batched", NULL, js_dbdsvdx, NULL, NULL, NULL, napi_default, NULL},
    {"dgesvdx_batched", NULL, js_dgesvdx, NULL, NULL, NULL, napi_default, NULL},
    {"dsyevxv_batched", NULL, js_dsyevxv, NULL, NULL, NULL, napi_default, NULL},
    {"dsygvx_batched", NULL, js_dsygvx, NULL, NULL, NULL, napi_default, NULL},
    {"dqp3rank_batched", NULL, js_dqp3rank, NULL, NULL, NULL, napi_default, NULL},
    {"dsrrqr_batched", NULL, js_dsrrqr, NULL, NULL, NULL, napi_default, NULL},
    {"durv_batched", NULL, js_durv, NULL, NULL, NULL, napi_default, NULL},
    {"durvls_batched", NULL, js_durvls, NULL, NULL, NULL, napi_default, NULL},
    {"dqp3ls_batched", NULL, js_dqp3ls, NULL, NULL, NULL, napi_default, NULL},
    {"dtrsm_batched", NULL, js_dtrsm, NULL, NULL, NULL, napi_default, NULL},
    {"dpotrf_batched", NULL, js_dpotrf, NULL, NULL, NULL, napi_default, NULL},
    {"dpotrs_batched", NULL, js_dpotrs, NULL, NULL, NULL, napi_default, NULL},
    {"dldltrf_batched", NULL, js_dldltrf, NULL, NULL, NULL, napi_default, NULL},
    {"dldltrs_batched", NULL, js_dldltrs, NULL, NULL, NULL, napi_default, NULL},
    {"dsytrf_bk_batched", NULL, js_dsytrf_bk, NULL, NULL, NULL, napi_default, NULL},
    {"dsytrs_bk_batched", NULL, js_dsytrs_bk, NULL, NULL, NULL, napi_default, NULL},
    {"dtranspose_batched", NULL, js_dtranspose, NULL, NULL, NULL, napi_default, NULL},
    {"dtri_batched", NULL, js_dtri, NULL, NULL, NULL, napi_default, NULL},
    {"ddiag_batched", NULL, js_ddiag, NULL, NULL, NULL, napi_default, NULL},
    {"ddiagmat_batched", NULL, js_ddiagmat, NULL, NULL, NULL, napi_default, NULL},
    {"dpermute_batched", NULL, js_dpermute, NULL, NULL, NULL, napi_default, NULL},
    {"gather_nd", NULL, js_gather_nd, NULL, NULL, NULL, napi_default, NULL},
    {"zip_nd", NULL, js_zip_nd, NULL, NULL, NULL, napi_default, NULL},
    {"reduce_nd", NULL, js_reduce_nd, NULL, NULL, NULL, napi_default, NULL},
    {"dev_alloc", NULL, js_dev_alloc, NULL, NULL, NULL, napi_default, NULL},
    {"dev_free", NULL, js_dev_free, NULL, NULL, NULL, napi_default, NULL},
    {"dev_upload", NULL, js_dev_upload, NULL, NULL, NULL, napi_default, NULL},
    {"dev_download", NULL, js_dev_download, NULL, NULL, NULL, napi_default, NULL},
    {"synchronize", NULL, js_synchronize, NULL, NULL, NULL, napi_default, NULL},
    {"profile_enable", NULL, js_profile_enable, NULL, NULL, NULL, napi_default, NULL},
    {"profile_last", NULL, js_profile_last, NULL, NULL, NULL, napi_default, NULL},
  };
  napi_define_properties(env, exports, sizeof props / sizeof props[0], props);
  napi_add_env_cleanup_hook(env, cleanup, NULL);
  return exports;
}
NAPI_MODULE(NODE_GYP_MODULE_NAME, init)

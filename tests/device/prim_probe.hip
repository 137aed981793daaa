// prim_probe DIR -- the math primitives of the kernels, run on the device on files of arguments.
//
// Reads DIR/exp64.arg, exp256.arg, log.arg, rcp.arg (raw fp64, written by tests/host/primitives_exact.cpp gen) and writes
// DIR/exp64.res, exp256.res, log.res, rcp64.res, rsqrt64.res, rr_inv.res, rr_rsq.res, fast_rcp.res and tables.res (et[64],
// et256[256], lt[128]).  tests/test_primitives.py runs it once and holds the results to long-double references.
// The functions and the tables are the shipped headers' own (k_render.h, k_split.h, device_common.h), compiled with the
// library's flags: one kernel per function, one thread per argument, the tables built in LDS by the kernels' recipes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/celeste_hip.h"
#include "k_render.h"
#include "k_split.h"

#define TRY(expr)                                                                                      \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            fprintf(stderr, "prim_probe: %s: %s\n", #expr, hipGetErrorString(e_));                     \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

enum { F_EXP64, F_EXP256, F_LOG, F_RCP64, F_RSQRT64, F_RR_INV, F_RR_RSQ, F_FAST_RCP };

// the tables as the kernels build them: et by the one-line recipe every kernel carries, et256 by exp_tab256_fill, lt from the
// constants cel_ctx_create uploads (log_tab_fill)
__device__ inline void probe_tables(double *et, double *et256, double *lt) {
    const int lane = threadIdx.x;
    if (lane < 64) {
        et[lane] = exp2((double)lane * (1.0 / 64.0));
        exp_tab256_fill(et256, lane, exp2((double)lane * (1.0 / 64.0)));
        lt[lane] = c_log_ic[lane];
        lt[64 + lane] = c_log_lc[lane];
    }
    __syncthreads();
}

template <int F>
__global__ void __launch_bounds__(256) k_probe(const double *__restrict__ arg, int64_t n, double *__restrict__ res) {
    __shared__ double et[64], et256[256], lt[128];
    probe_tables(et, et256, lt);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = arg[i];
    double r, o;
    if (F == F_EXP64) r = exp_tab64(x, et);
    else if (F == F_EXP256) r = exp_tab256_p3(x, et256);
    else if (F == F_LOG) r = log_tab(x, lt);
    else if (F == F_RCP64) r = rcp64(x);
    else if (F == F_RSQRT64) r = rsqrt64(x);
    else if (F == F_RR_INV) rcp_rsqrt(x, r, o);
    else if (F == F_RR_RSQ) rcp_rsqrt(x, o, r);
    else r = fast_rcp(x);
    res[i] = r;
}

__global__ void __launch_bounds__(256) k_probe_tables(double *__restrict__ out /* 448 */) {
    __shared__ double et[64], et256[256], lt[128];
    probe_tables(et, et256, lt);
    const int t = threadIdx.x;
    if (t < 64) out[t] = et[t];
    out[64 + t] = et256[t];
    if (t < 128) out[320 + t] = lt[t];
}

static bool read_file(const std::string &p, std::vector<double> &v) {
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t)sz / 8);
    const size_t got = fread(v.data(), 8, v.size(), f);
    fclose(f);
    return got == v.size() && !v.empty();
}
static bool write_file(const std::string &p, const double *v, size_t n) {
    FILE *f = fopen(p.c_str(), "wb");
    if (!f) return false;
    const size_t put = fwrite(v, 8, n, f);
    return fclose(f) == 0 && put == n;
}

template <int F>
static int run(const std::string &dir, const std::vector<double> &arg, const char *name, double *d_arg, double *d_res, std::vector<double> &res) {
    const int64_t n = (int64_t)arg.size();
    hipLaunchKernelGGL(k_probe<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_arg, n, d_res);
    TRY(hipGetLastError());
    TRY(hipMemcpy(res.data(), d_res, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (!write_file(dir + "/" + name + ".res", res.data(), (size_t)n)) { fprintf(stderr, "prim_probe: cannot write %s.res\n", name); return 1; }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: prim_probe DIR\n"); return 2; }
    const std::string dir = argv[1];
    std::vector<double> a64, a256, alog, arcp;
    if (!read_file(dir + "/exp64.arg", a64) || !read_file(dir + "/exp256.arg", a256) || !read_file(dir + "/log.arg", alog) ||
        !read_file(dir + "/rcp.arg", arcp)) {
        fprintf(stderr, "prim_probe: argument files missing in %s\n", dir.c_str());
        return 2;
    }
    size_t cap = 448;
    for (const auto *v : {&a64, &a256, &alog, &arcp}) cap = v->size() > cap ? v->size() : cap;
    TRY(hipSetDevice(0));
    double ic[64], lc[64];
    log_tab_fill(ic, lc);
    TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_log_ic), ic, sizeof(ic)));
    TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_log_lc), lc, sizeof(lc)));
    double *d_arg = nullptr, *d_res = nullptr;
    TRY(hipMalloc(&d_arg, sizeof(double) * cap));
    TRY(hipMalloc(&d_res, sizeof(double) * cap));
    std::vector<double> res(cap);
    hipLaunchKernelGGL(k_probe_tables, dim3(1), dim3(256), 0, 0, d_res);
    TRY(hipGetLastError());
    TRY(hipMemcpy(res.data(), d_res, sizeof(double) * 448, hipMemcpyDeviceToHost));
    if (!write_file(dir + "/tables.res", res.data(), 448)) return 1;
    int rc = 0;
    TRY(hipMemcpy(d_arg, a64.data(), sizeof(double) * a64.size(), hipMemcpyHostToDevice));
    if ((rc = run<F_EXP64>(dir, a64, "exp64", d_arg, d_res, res))) return rc;
    TRY(hipMemcpy(d_arg, a256.data(), sizeof(double) * a256.size(), hipMemcpyHostToDevice));
    if ((rc = run<F_EXP256>(dir, a256, "exp256", d_arg, d_res, res))) return rc;
    TRY(hipMemcpy(d_arg, alog.data(), sizeof(double) * alog.size(), hipMemcpyHostToDevice));
    if ((rc = run<F_LOG>(dir, alog, "log", d_arg, d_res, res))) return rc;
    TRY(hipMemcpy(d_arg, arcp.data(), sizeof(double) * arcp.size(), hipMemcpyHostToDevice));
    if ((rc = run<F_RCP64>(dir, arcp, "rcp64", d_arg, d_res, res))) return rc;
    if ((rc = run<F_RSQRT64>(dir, arcp, "rsqrt64", d_arg, d_res, res))) return rc;
    if ((rc = run<F_RR_INV>(dir, arcp, "rr_inv", d_arg, d_res, res))) return rc;
    if ((rc = run<F_RR_RSQ>(dir, arcp, "rr_rsq", d_arg, d_res, res))) return rc;
    if ((rc = run<F_FAST_RCP>(dir, arcp, "fast_rcp", d_arg, d_res, res))) return rc;
    TRY(hipFree(d_arg));
    TRY(hipFree(d_res));
    printf("prim_probe: %zu + %zu + %zu + 5 x %zu results\n", a64.size(), a256.size(), alog.size(), arcp.size());
    return 0;
}

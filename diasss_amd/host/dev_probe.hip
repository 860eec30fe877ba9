// diasss_amd/host/dev_probe.hip -- the kernels' shared __device__ helpers, evaluated ON THE DEVICE one function at a time.
// Includes the headers as the kernels do and is built with the library's code-generation flags, so every number it writes is the number a
// kernel would compute.  tests/test_gpu_dev_probe.py compares them with the oracle, with 50-digit references and with numpy restatements.
// Nothing here judges a number.  Stand-alone (own main, not part of libdsss.so); every HIP call is checked, the first error is printed and
// ends the program non-zero with nothing further launched; without a device it exits 77.
//
//     dev_probe IN OUT           IN: records of 64 doubles [function id, 63 inputs (unused ones zero)], OUT: 48 doubles per record (unused ones zero)
//                                one launch per function id, one thread per record
//     id  function                 inputs                                   outputs
//   0-11  as host/pose_check.cpp (so3_exp ... the Between factor's error chain), same inputs and outputs
//     12  sss_factor               p[3] T[12] mx my                         e[2] H1[6] H2[12]
//     13  dsss_sincos              m <= 24, x[m]                            (s c)[m]         (the long lists share records: the same calls, fewer bytes)
//     14  dsss_geo_at              pose row[6] M col gr[M / 2], M <= 32     x y
//     15  fast_atan2_dev           m <= 31, (y x)[m] (floats as doubles)    angle[m]
//     16  factor_eval<true>        Xa[12] Xb[12] meas[12] w[6]              r[6] Ji[36]      (the Between form: k = 1 of n = 2)
//     17  chol6_recip              A[36]                                    A'[36] ri[6] bad
//     18  chol6_rdiag              A[36]                                    A'[36] bad
//     19  the LM rule              kind (0 verdict, 1 lambda, 2 continue), row of host/lm_rule_table.h
//                                  -> rows of that kind, 1 if the row exists, got[3], expected[3]
//                                     verdict: descends success stop; lambda: early give-ups, gives up, next lambda (expected < 0: not stated);
//                                     continue: go, 0, 0
//
//     dev_probe --scan IN OUT    the order-sensitive collectives of csrc/dsss_wave.h and block_sum256 on vectors.
//                                IN: sections [int64 type (0 int32, 1 uint64, 2 f64), int64 n, n elements of 8 bytes (int32 as int64)]
//                                OUT per section, 8 bytes per element, P = n rounded up to 256:
//                                  n exclusive prefixes and the total of dsss_block_scan_excl<4> carried over chunks of 256 by one workgroup,
//                                  P dsss_wave_scan_incl, P / 64 dsss_wave_sum (lanes past n hold 0), and for f64 P / 256 block_sum256
#include "../csrc/dsss_internal.h"
#include "../csrc/dsss_pose.h"
#include "../csrc/dsss_lm.h"
#include "../csrc/dsss_extract.h"
#include "../csrc/dsss_wave.h"
#include "../csrc/dsss_pg_dev.h"
#include "lm_rule_table.h"
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

enum { IN_W = 64, OUT_W = 48, N_IDS = 20, MAX_M = 32, SINCOS_PER_REC = 24, ATAN2_PER_REC = 31 };

#define HIP_OK(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) { \
    std::printf("dev_probe: %s failed: %s\n", #call, hipGetErrorString(e_)); return 1; } } while (0)

__device__ inline pose_t get_pose(const double* p)
{
    pose_t T;
    for (int i = 0; i < 9; ++i) T.R[i] = p[i];
    for (int i = 0; i < 3; ++i) T.t[i] = p[9 + i];
    return T;
}
__device__ inline void put_pose(const pose_t& T, double* o)
{
    for (int i = 0; i < 9; ++i) o[i] = T.R[i];
    for (int i = 0; i < 3; ++i) o[9 + i] = T.t[i];
}

template <int ID>
__device__ inline void eval(const double* a, double* out)
{
    if constexpr (ID == 0) so3_exp(a, out);
    else if constexpr (ID == 1) so3_log(a, out);
    else if constexpr (ID == 2) { pose_t O; pose_exp(a, &O); put_pose(O, out); }
    else if constexpr (ID == 3) { const pose_t A = get_pose(a); pose_log(&A, out); }
    else if constexpr (ID == 4) { pose_t O; const pose_t A = get_pose(a), B = get_pose(a + 12); pose_between(&A, &B, &O); put_pose(O, out); }
    else if constexpr (ID == 5) { pose_t O; const pose_t A = get_pose(a); pose_inverse(&A, &O); put_pose(O, out); }
    else if constexpr (ID == 6) { pose_t O; const pose_t A = get_pose(a), B = get_pose(a + 12); pose_compose(&A, &B, &O); put_pose(O, out); }
    else if constexpr (ID == 7) { const pose_t A = get_pose(a); pose_adjoint(&A, out); }
    else if constexpr (ID == 8) { pose_t O; const pose_t A = get_pose(a); pose_retract(&A, a + 12, &O); put_pose(O, out); }
    else if constexpr (ID == 9) { const pose_t A = get_pose(a); pose_rpy(&A, out); }
    else if constexpr (ID == 10) { pose_t O; pose_from_rodrigues(a, &O); put_pose(O, out); }
    else if constexpr (ID == 11) {
        pose_t H, O; const pose_t A = get_pose(a), B = get_pose(a + 12), M = get_pose(a + 24);
        pose_between(&A, &B, &H); pose_between(&M, &H, &O); pose_log(&O, out);
    }
    else if constexpr (ID == 12) { const pose_t A = get_pose(a + 3); sss_factor(a, &A, a[15], a[16], out, out + 2, out + 8); }
    else if constexpr (ID == 13) {
        int m = (int)a[0]; if (m < 0) m = 0; if (m > SINCOS_PER_REC) m = SINCOS_PER_REC;
        for (int i = 0; i < m; ++i) dsss_sincos(a[1 + i], out + 2 * i, out + 2 * i + 1);
    }
    else if constexpr (ID == 14) {
        int m = (int)a[6]; if (m < 2) m = 2; if (m > MAX_M) m = MAX_M;      // the record holds MAX_M / 2 ground ranges at most
        int col = (int)a[7]; if (col < 0) col = 0; if (col > m - 1) col = m - 1;
        dsss_geo_at(a, a + 8, m, 0, col, out, out + 1);
    }
    else if constexpr (ID == 15) {
        int m = (int)a[0]; if (m < 0) m = 0; if (m > ATAN2_PER_REC) m = ATAN2_PER_REC;
        for (int i = 0; i < m; ++i) out[i] = (double)fast_atan2_dev((float)a[1 + 2 * i], (float)a[2 + 2 * i]);
    }
    else if constexpr (ID == 16) {
        pose_t X[2] = { get_pose(a), get_pose(a + 12) }, meas[2];
        pose_identity(&meas[0]); meas[1] = get_pose(a + 24);
        pg_weights W;
        for (int i = 0; i < 6; ++i) { W.prior[i] = 0.0; W.odo[i] = a[36 + i]; }
        double r[6], Ji[36];
        factor_eval<true>(1, 2, X, meas, W, nullptr, nullptr, nullptr, nullptr, r, Ji);
        for (int i = 0; i < 6; ++i) out[i] = r[i];
        for (int i = 0; i < 36; ++i) out[6 + i] = Ji[i];
    }
    else if constexpr (ID == 17) {
        double S[36], ri[6];
        for (int i = 0; i < 36; ++i) S[i] = a[i];
        const int bad = chol6_recip(S, ri);
        for (int i = 0; i < 36; ++i) out[i] = S[i];
        for (int i = 0; i < 6; ++i) out[36 + i] = ri[i];
        out[42] = bad;
    }
    else if constexpr (ID == 18) {
        double S[36];
        for (int i = 0; i < 36; ++i) S[i] = a[i];
        const int bad = chol6_rdiag(S);
        for (int i = 0; i < 36; ++i) out[i] = S[i];
        out[36] = bad;
    }
    else if constexpr (ID == 19) {
        const int kind = (int)a[0], row = (int)a[1];
        const int rows = kind == 0 ? (int)LM_VERDICT_ROWS : kind == 1 ? (int)LM_LAMBDA_ROWS : kind == 2 ? (int)LM_CONTINUE_ROWS : 0;
        out[0] = rows;
        if (row < 0 || row >= rows) return;
        out[1] = 1;
        if (kind == 0) {
            const lm_verdict_row V = lm_table_verdict(row);
            const lm_verdict v = lm_judge(lm_table_rule(V.rule), V.oldLin, V.newLin, V.err, V.newErr);
            out[2] = lm_descends(V.oldLin, V.newLin); out[3] = v.success; out[4] = v.stop;
            out[5] = V.descends; out[6] = V.success; out[7] = V.stop;
        } else if (kind == 1) {
            const lm_lambda_row S = lm_table_lambda(row);
            const lm_lambda_got g = lm_table_lambda_run(S);
            out[2] = g.early; out[3] = g.gave_up; out[4] = g.next;
            out[5] = 0; out[6] = S.gives_up; out[7] = S.next;
        } else {
            const lm_continue_row C = lm_table_continue(row);
            out[2] = lm_continue(lm_table_rule(C.rule), C.iters, C.cur, C.err);
            out[5] = C.go;
        }
    }
}

// one thread per record of function ID; which[] lists the records.  Reads and writes its own record only.
template <int ID>
__global__ __launch_bounds__(64) void probe_kernel(const double* __restrict__ in, double* __restrict__ out, const int* __restrict__ which, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const size_t r = (size_t)which[i];
    eval<ID>(in + r * IN_W + 1, out + r * OUT_W);
}

template <int ID>
static hipError_t launch_from(int id, const double* in, double* out, const int* which, int n)
{
    if constexpr (ID < N_IDS) {
        if (id != ID) return launch_from<ID + 1>(id, in, out, which, n);
        probe_kernel<ID><<<dim3((unsigned)((n + 63) / 64)), dim3(64)>>>(in, out, which, n);
        return hipGetLastError();
    } else return hipErrorInvalidValue;
}

static bool read_file(const char* path, std::vector<unsigned char>* bytes)
{
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) bytes->insert(bytes->end(), buf, buf + got);
    const bool ok = !std::ferror(f);
    std::fclose(f);
    return ok;
}
static bool write_file(const char* path, const void* p, size_t bytes)
{
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
    return (std::fclose(f) == 0) && ok;
}

static int run_records(const char* fin, const char* fout)
{
    std::vector<unsigned char> bytes;
    if (!read_file(fin, &bytes)) { std::printf("dev_probe: cannot read %s\n", fin); return 2; }
    if (bytes.size() % (IN_W * sizeof(double)) != 0) { std::printf("dev_probe: %s is not a whole number of records\n", fin); return 2; }
    const size_t n = bytes.size() / (IN_W * sizeof(double));
    if (n > (size_t)1 << 24) { std::printf("dev_probe: too many records\n"); return 2; }
    std::vector<double> in(n * IN_W + 1);
    std::memcpy(in.data(), bytes.data(), bytes.size());
    std::vector<std::vector<int>> by_id(N_IDS);
    for (size_t i = 0; i < n; ++i) {
        const double id = in[i * IN_W];
        if (!(id >= 0 && id < N_IDS && id == (double)(int)id)) { std::printf("dev_probe: record %zu: unknown function id %g\n", i, id); return 1; }
        by_id[(int)id].push_back((int)i);
    }
    std::vector<double> out(n * OUT_W + 1, 0.0);
    double *d_in = nullptr, *d_out = nullptr; int* d_which = nullptr;
    HIP_OK(hipMalloc(&d_in, (n * IN_W + 1) * sizeof(double)));
    HIP_OK(hipMalloc(&d_out, (n * OUT_W + 1) * sizeof(double)));
    HIP_OK(hipMalloc(&d_which, (n + 1) * sizeof(int)));
    HIP_OK(hipMemcpy(d_in, in.data(), n * IN_W * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0, (n * OUT_W + 1) * sizeof(double)));
    for (int id = 0; id < N_IDS; ++id) {
        const int m = (int)by_id[id].size();
        if (m == 0) continue;
        HIP_OK(hipMemcpy(d_which, by_id[id].data(), m * sizeof(int), hipMemcpyHostToDevice));
        HIP_OK(launch_from<0>(id, d_in, d_out, d_which, m));
        HIP_OK(hipDeviceSynchronize());
    }
    HIP_OK(hipMemcpy(out.data(), d_out, n * OUT_W * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_in)); HIP_OK(hipFree(d_out)); HIP_OK(hipFree(d_which));
    if (!write_file(fout, out.data(), n * OUT_W * sizeof(double))) { std::printf("dev_probe: cannot write %s\n", fout); return 2; }
    std::printf("dev_probe: ok, %zu records\n", n);
    return 0;
}

// ------------------------------------------------------------------ the collectives
// one workgroup of 256 carries the scan over chunks of 256, as scan_counts_kernel and pg_compact_block carry it
template <typename T>
__global__ __launch_bounds__(256) void carried_scan_kernel(const T* __restrict__ v, long long n, T* __restrict__ prefix)
{
    __shared__ T s_w[4];
    T base = 0;
    for (long long c0 = 0; c0 < n; c0 += 256) {
        const long long i = c0 + threadIdx.x;
        const T x = i < n ? v[i] : (T)0;
        T tot;
        const T p = dsss_block_scan_excl<4, T>(x, &tot, s_w);
        if (i < n) prefix[i] = base + p;
        base += tot;
    }
    if (threadIdx.x == 0) prefix[n] = base;
}
// per wavefront the inclusive scan and the sum, per workgroup of 256 the block sum (f64 only); v is padded with zeros to P = gridDim.x * 256
template <typename T>
__global__ __launch_bounds__(256) void wave_kernel(const T* __restrict__ v, T* __restrict__ incl, T* __restrict__ wsum, double* __restrict__ bsum)
{
    __shared__ double s_w[4];
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const T x = v[i];
    incl[i] = dsss_wave_scan_incl(x);
    const T s = dsss_wave_sum(x);
    if ((threadIdx.x & 63) == 0) wsum[i >> 6] = s;
    if constexpr (std::is_same<T, double>::value) {
        const double b = block_sum256(x, s_w);
        if (threadIdx.x == 0) bsum[blockIdx.x] = b;
    }
}

template <typename T>
static int scan_section(const int64_t* src, long long n, bool is_f64, std::vector<int64_t>* outv)
{
    const long long P = (n + 255) / 256 * 256, nw = P / 64, nb = P / 256;
    std::vector<T> h(P, (T)0);
    for (long long i = 0; i < n; ++i) {
        if constexpr (sizeof(T) == 4) h[i] = (T)src[i];
        else std::memcpy(&h[i], &src[i], 8);
    }
    T *d_v = nullptr, *d_prefix = nullptr, *d_incl = nullptr, *d_wsum = nullptr; double* d_bsum = nullptr;
    HIP_OK(hipMalloc(&d_v, P * sizeof(T)));
    HIP_OK(hipMalloc(&d_prefix, (n + 1) * sizeof(T)));
    HIP_OK(hipMalloc(&d_incl, P * sizeof(T)));
    HIP_OK(hipMalloc(&d_wsum, nw * sizeof(T)));
    HIP_OK(hipMalloc(&d_bsum, nb * sizeof(double)));
    HIP_OK(hipMemcpy(d_v, h.data(), P * sizeof(T), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_bsum, 0, nb * sizeof(double)));
    carried_scan_kernel<T><<<dim3(1), dim3(256)>>>(d_v, n, d_prefix);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    wave_kernel<T><<<dim3((unsigned)nb), dim3(256)>>>(d_v, d_incl, d_wsum, d_bsum);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<T> prefix(n + 1), incl(P), wsum(nw); std::vector<double> bsum(nb);
    HIP_OK(hipMemcpy(prefix.data(), d_prefix, (n + 1) * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(incl.data(), d_incl, P * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(wsum.data(), d_wsum, nw * sizeof(T), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(bsum.data(), d_bsum, nb * sizeof(double), hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_v)); HIP_OK(hipFree(d_prefix)); HIP_OK(hipFree(d_incl)); HIP_OK(hipFree(d_wsum)); HIP_OK(hipFree(d_bsum));
    auto put = [&](const T& x) { int64_t w; if constexpr (sizeof(T) == 4) w = (int64_t)x; else std::memcpy(&w, &x, 8); outv->push_back(w); };
    for (const T& x : prefix) put(x);
    for (const T& x : incl) put(x);
    for (const T& x : wsum) put(x);
    if (is_f64) for (double x : bsum) { int64_t w; std::memcpy(&w, &x, 8); outv->push_back(w); }
    return 0;
}

static int run_scan(const char* fin, const char* fout)
{
    std::vector<unsigned char> bytes;
    if (!read_file(fin, &bytes)) { std::printf("dev_probe: cannot read %s\n", fin); return 2; }
    if (bytes.size() % 8 != 0) { std::printf("dev_probe: %s is not a whole number of 8-byte words\n", fin); return 2; }
    std::vector<int64_t> w(bytes.size() / 8 + 1);
    std::memcpy(w.data(), bytes.data(), bytes.size());
    const size_t nwords = bytes.size() / 8;
    std::vector<int64_t> outv;
    size_t at = 0; int sections = 0;
    while (at < nwords) {
        if (at + 2 > nwords) { std::printf("dev_probe: %s ends inside a section header\n", fin); return 2; }
        const int64_t type = w[at], n = w[at + 1];
        if (type < 0 || type > 2 || n < 1 || n > (1 << 24) || at + 2 + (size_t)n > nwords) { std::printf("dev_probe: section %d: bad header\n", sections); return 2; }
        const int64_t* src = &w[at + 2];
        const int rc = type == 0 ? scan_section<int32_t>(src, n, false, &outv) : type == 1 ? scan_section<uint64_t>(src, n, false, &outv)
                                                                                            : scan_section<double>(src, n, true, &outv);
        if (rc) return rc;
        at += 2 + (size_t)n; ++sections;
    }
    if (!write_file(fout, outv.data(), outv.size() * 8)) { std::printf("dev_probe: cannot write %s\n", fout); return 2; }
    std::printf("dev_probe: ok, %d sections\n", sections);
    return 0;
}

int main(int argc, char** argv)
{
    const bool scan = argc == 4 && std::strcmp(argv[1], "--scan") == 0;
    if (!scan && argc != 3) { std::printf("usage: dev_probe IN OUT | dev_probe --scan IN OUT\n"); return 2; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { std::printf("dev_probe: no device\n"); return 77; }
    return scan ? run_scan(argv[2], argv[3]) : run_records(argv[1], argv[2]);
}

// tools/sqrt_check.hip -- hpe_sqrt, hpe_sqrt_nr and hpe_sqrt_direct (hpe_device.hpp), bitwise.
// Three checks, exit status 0 only if every one finds no mismatch:
//   1. hpe_sqrt against the host's std::sqrt (IEEE-754: correctly rounded, so a reference
//      that owes nothing to the device compiler) on 2^20 inputs: the special cases, squared
//      distances in [0, 1e4) cm^2 and the exponents around the 2^-767 bound;
//   2. on the same inputs, hpe_sqrt_direct against its claim (true exactly for
//      2^-767 <= x < inf) and, where it is true, hpe_sqrt_nr ALONE against std::sqrt;
//   3. hpe_sqrt against the device compiler's sqrt on 2^22 random bit patterns of every
//      exponent (NaN payloads and signs included, compared bit for bit).
// Two NaNs count as equal in 1 and 2 (the host's and the device's default NaN differ in sign).
// Build: make -C hand-pose-estimation_amd sqrt_check (the library's device flags)
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <cmath>
#include <vector>
#include "../hand-pose-estimation_amd/csrc/hpe_device.hpp"

#define CHK(call)                                                                       \
    do {                                                                                \
        const hipError_t e_ = (call);                                                   \
        if (e_ != hipSuccess) {                                                         \
            std::fprintf(stderr, "sqrt_check: %s: %s\n", #call, hipGetErrorString(e_)); \
            return 2;                                                                   \
        }                                                                               \
    } while (0)

__global__ void k_check(const double *a, unsigned long long *bad, double *first, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    const double s1 = __builtin_sqrt(x), s2 = hpe_sqrt(x);
    if (__double_as_longlong(s1) != __double_as_longlong(s2)) {
        if (atomicAdd(bad, 1ull) == 0) *first = x;
    }
}

// the values themselves, for the host to judge
__global__ void k_roots(const double *a, double *full, double *nr, unsigned char *direct, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    full[i] = hpe_sqrt(x);
    nr[i] = hpe_sqrt_nr(x);
    direct[i] = hpe_sqrt_direct(x) ? 1 : 0;
}

static uint64_t bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}
static bool same(double got, double want) {
    return (std::isnan(got) && std::isnan(want)) || bits(got) == bits(want);
}

int main() {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    const double sp[] = {0.0, -0.0, INFINITY, -INFINITY, NAN, -NAN, 0x1p-767, 0x1p-768, 0x1p-1074,
                         0x1.fffffffffffffp-768, 0x1.0000000000001p-767, 0x1.fffffffffffffp+1023,
                         0x1p-1022, 0x1.fffffffffffffp-1023, 0x1p-766, 1.0, 2.0, 4.0, -1.0,
                         -0x1p-767, -0x1p-1074, 0x1.fffffffffffffp-1, 0x1.0000000000001p+0};
    const int nsp = (int)(sizeof(sp) / sizeof(sp[0]));

    // ---- 1 and 2: against the host's sqrt
    const int m = 1 << 20;
    std::vector<double> hm(m);
    for (int i = 0; i < m; ++i) {
        const uint64_t r = rnd();
        if (i % 2 == 0) hm[i] = (double)(r >> 11) * 0x1p-53 * 1e4;  // d2 in [0, 1e4) cm^2
        else hm[i] = std::ldexp(1.0 + (double)(r >> 12) * 0x1p-52, -767 + (int)(r % 8) - 4);
    }
    for (int k = 0; k < nsp; ++k) hm[k] = sp[k];
    double *dm, *dfull, *dnr;
    unsigned char *ddir;
    CHK(hipMalloc(&dm, sizeof(double) * m));
    CHK(hipMalloc(&dfull, sizeof(double) * m));
    CHK(hipMalloc(&dnr, sizeof(double) * m));
    CHK(hipMalloc(&ddir, m));
    CHK(hipMemcpy(dm, hm.data(), sizeof(double) * m, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_roots, dim3((m + 255) / 256), dim3(256), 0, 0, dm, dfull, dnr, ddir, m);
    CHK(hipGetLastError());
    std::vector<double> full(m), nr(m);
    std::vector<unsigned char> dir(m);
    CHK(hipMemcpy(full.data(), dfull, sizeof(double) * m, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(nr.data(), dnr, sizeof(double) * m, hipMemcpyDeviceToHost));
    CHK(hipMemcpy(dir.data(), ddir, m, hipMemcpyDeviceToHost));
    unsigned long long bad_full = 0, bad_nr = 0, bad_dir = 0, n_dir = 0;
    double f_full = 0, f_nr = 0, f_dir = 0;
    for (int i = 0; i < m; ++i) {
        const double x = hm[i];
        const volatile double xv = x;  // no compile-time folding of the reference
        const double want = std::sqrt(xv);
        if (!same(full[i], want) && bad_full++ == 0) f_full = x;
        const bool claim = x >= 0x1p-767 && x < INFINITY;  // false for NaN
        if ((dir[i] != 0) != claim && bad_dir++ == 0) f_dir = x;
        if (dir[i]) {
            ++n_dir;
            if (!same(nr[i], want) && bad_nr++ == 0) f_nr = x;
        }
    }
    std::printf("hpe_sqrt vs host sqrt: %d inputs, %llu bitwise mismatches", m, bad_full);
    if (bad_full) std::printf(" (first %a)", f_full);
    std::printf("\n");
    std::printf("hpe_sqrt_direct vs 2^-767 <= x < inf: %d inputs, %llu mismatches", m, bad_dir);
    if (bad_dir) std::printf(" (first %a)", f_dir);
    std::printf("\n");
    std::printf("hpe_sqrt_nr vs host sqrt where direct: %llu inputs, %llu bitwise mismatches", n_dir,
                bad_nr);
    if (bad_nr) std::printf(" (first %a)", f_nr);
    std::printf("\n");

    // ---- 3: against the device compiler's sqrt
    const int n = 1 << 22;
    std::vector<double> h(n);
    for (int i = 0; i < n; ++i) {
        const uint64_t r = rnd();
        double v;
        switch (i % 4) {
        case 0: std::memcpy(&v, &r, 8); break;                         // any bit pattern
        case 1: v = (double)(r >> 11) * 0x1p-53 * 1e4; break;          // d2 in [0, 1e4) cm^2
        case 2: v = std::ldexp(1.0 + (double)(r >> 12) * 0x1p-52, -767 + (int)(r % 8) - 4); break;
        default: v = std::ldexp(1.0 + (double)(r >> 12) * 0x1p-52, (int)(r % 2098) - 1074); break;
        }
        h[i] = v;
    }
    for (int k = 0; k < nsp; ++k) h[k] = sp[k];
    double *da, *df;
    unsigned long long *db;
    CHK(hipMalloc(&da, sizeof(double) * n));
    CHK(hipMalloc(&df, sizeof(double)));
    CHK(hipMalloc(&db, sizeof(unsigned long long)));
    CHK(hipMemcpy(da, h.data(), sizeof(double) * n, hipMemcpyHostToDevice));
    CHK(hipMemset(db, 0, sizeof(unsigned long long)));
    CHK(hipMemset(df, 0, sizeof(double)));
    hipLaunchKernelGGL(k_check, dim3((n + 255) / 256), dim3(256), 0, 0, da, db, df, n);
    CHK(hipGetLastError());
    unsigned long long bad = 0;
    double first = 0;
    CHK(hipMemcpy(&bad, db, sizeof(bad), hipMemcpyDeviceToHost));
    CHK(hipMemcpy(&first, df, sizeof(first), hipMemcpyDeviceToHost));
    std::printf("hpe_sqrt vs device sqrt: %d inputs, %llu bitwise mismatches", n, bad);
    if (bad) std::printf(" (first %a)", first);
    std::printf("\n");
    return (bad || bad_full || bad_nr || bad_dir) ? 1 : 0;
}

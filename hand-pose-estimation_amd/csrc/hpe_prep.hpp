// hpe_prep.hpp -- observedmodel preprocessing on the GPU:
//   depth mm -> cm                                   (observedmodel.cpp:296-308)
//   point cloud of the non-zero pixels, row-major    (observedmodel.cpp:110-169)
//   cm-per-pixel scale = mean of 2 / |d(u,v)|        (observedmodel.cpp:171-202)
//   down-sample to rows k * floor(N / 250)           (observedmodel.cpp:204-217)
//   5x5 chamfer distance transform of the background (observedmodel.cpp:313-358,
//     OpenCV distanceTransform(CV_DIST_L2, 5): 16.16 fixed point, weights 1 / 1.4 / 2.1969)
//
// Workgroups (PREP_WG of them, PREP_NT threads each, in one launch):
//   PREP_BANDS "band" workgroups: 30 image rows each -- depth, per-pixel cloud point and
//     scale term, compacted in pixel order within the band.  The last band to finish
//     merges: band offsets, the scale mean replayed in Armadillo's order (two alternating
//     sequential accumulators), the (down-sampled) cloud.
//   one DT workgroup: the chamfer raster scans by ONE wave, lane l holding columns
//     5l..5l+4, rows in registers; the in-row dependency T_c = min(a_c, T_{c-1} + 1) is a
//     prefix minimum (lane-serial over 5 columns, DPP across lanes).  Integer min-plus
//     arithmetic: exactly the raster-scan values.  Resident raw sequences split the two
//     scans over consecutive launches, on two waves (prep_dt_split).
// Results equal hpe_preprocess_depth bit for bit.  Hand-offs between workgroups follow
// MI355X_MICROARCH.md (inter-workgroup visibility): every storing wave waits for its
// stores, workgroup barrier, agent release, arrival counter; the last arriver acquires.
#pragma once
#include "hpe_device.hpp"
#include "../../include/hpe.h"

#define PREP_NT 512
#define PREP_BANDS 8
#define PREP_WG (PREP_BANDS + 1)
#define PREP_ROWS (HPE_IMG_H / PREP_BANDS)      // 30
#define PREP_BAND_PIX (PREP_ROWS * HPE_IMG_W)  // 9600
#define PREP_CH 4096                           // scale terms staged in LDS per pass
#define DT_HV 65536
#define DT_DIAG 91750
#define DT_LONG 143976
#define DT_INIT (0x7FFFFFFF >> 2)

struct PrepInfo {
    int n_full, n;
    double scale, dtmax;
    int band_n[PREP_BANDS], band_h[PREP_BANDS];  // points / scale terms per band
};

// Arguments of one frame preparation (device pointers of the destination slot).
struct PrepArgs {
    const float *raw;
    int to_cm, downsample;
    double focal;
    double *depth_cm, *cx, *cy, *cz, *tmp, *ctb;
    float *dt;
    int *dtf;
    PrepInfo *info;
    DevObs *obs_out;
    unsigned *ctr;  // [0] bands arrived, [1] (merged cloud, DT) arrived, [2] DT has its mask
    // resident raw sequences (hpe_track_raw_sequence_dev): raw is the sequence's first frame
    // and the frame prepared is the one after the device row cursor's (*raw_row + 1), so a
    // captured chunk graph serves every chunk; null: raw is the frame itself
    const int *raw_row;
    unsigned long long raw_stride;  // floats per raw frame
};

// The same for a frame of 16-bit pixels (the live batch's u16 lanes, include/hpe.h): raw names
// 240x320 unsigned 16-bit values, and pixel value u stands for the raw float (float)u * unit --
// one fp32 multiply, 0 stays 0 -- on which everything downstream is the float forms' code.  The
// argument type selects the typed load (raw_load / raw_value below): prep_workgroup, prep_band
// and prep_dt are templates on it, and the float forms compile as before.
struct PrepArgsU16 : PrepArgs {
    float unit;  // the batch's depth unit in mm, read from device memory by the kernel
};
__device__ __forceinline__ float raw_load(const PrepArgs &a, int i) { return a.raw[i]; }
__device__ __forceinline__ float raw_value(const PrepArgs &, float r) { return r; }
// an unsigned load: values above 32767 are depths like the others
__device__ __forceinline__ unsigned short raw_load(const PrepArgsU16 &a, int i) {
    return ((const unsigned short *)a.raw)[i];
}
__device__ __forceinline__ float raw_value(const PrepArgsU16 &a, unsigned short u) {
    return (float)u * a.unit;
}

// The same through a lane view (hpe_view, include/hpe.h "Lane views"): raw names a camera frame
// of pitch x height 16-bit pixels, and model pixel i = 320 r + c stands for camera pixel
// (row0 + step r, col0 + step (FLIP ? 319 - c : c)), or for 0 when that lies outside the camera
// image.  view_pick is the rule's index arithmetic, shared with the locate kernel: the index is
// clamped into the image, so the load is unconditional, and a select zeroes what lay outside --
// no load becomes conditional, and all of prep_band's passes stay in flight at once.  The value
// that is left then takes the u16 rule, (float)u * unit.
struct PrepArgsView : PrepArgsU16 {
    hpe_view view;  // the lane's entry of the device table the begin wrote
};
// What a view batch's kernels receive where a u16 batch's receive the address of its depth unit:
// the unit, and behind it the lanes' views -- one block of device memory the begin writes, so the
// lane kernels keep one argument list and no graph holds a view.
struct ViewTab {
    float unit;
    int pad[7];
    hpe_view view[HPE_BATCH_MAX];
};
static_assert(sizeof(hpe_view) == 32 && offsetof(ViewTab, view) == 32, "hpe_view is 32 bytes");
__device__ __forceinline__ int view_pick(const hpe_view &v, int i, bool *inside) {
    const int r = i / HPE_IMG_W, c = i - HPE_IMG_W * r;
    // (unsigned adds: an origin near INT_MAX wraps to a negative coordinate, outside like the sum)
    const int cc = (v.flags & HPE_VIEW_FLIP_COLS) ? HPE_IMG_W - 1 - c : c;
    const int sr = (int)((unsigned)v.row0 + (unsigned)(v.step * r));
    const int sc = (int)((unsigned)v.col0 + (unsigned)(v.step * cc));
    *inside = (unsigned)sr < (unsigned)v.height && (unsigned)sc < (unsigned)v.width;
    return min(max(sr, 0), v.height - 1) * v.pitch + min(max(sc, 0), v.width - 1);
}
// A loaded view pixel: the 16 bits the clamped load brought, and the model pixel they were
// picked for -- a compile-time expression of the thread index once the passes are unrolled, so
// it takes no register.  raw_value selects: whether the pick lay inside the camera image is
// computed again where the value is used, beside the window's own row and column arithmetic,
// and nothing but the 16 bits is carried across the load's latency.  (The pick at the load is
// made on an opaque copy of i: merged with the one at the use by the compiler, its row, column
// and flag would stay live in registers for every load in flight, and the forms spill.)
struct ViewPix {
    unsigned short u;
    int i;
};
__device__ __forceinline__ ViewPix raw_load(const PrepArgsView &a, int i) {
    int j = i;
    asm("" : "+v"(j));
    bool inside;
    // an unsigned 32-bit byte offset on the lane's uniform base: one address register per load
    const unsigned off = 2u * (unsigned)view_pick(a.view, j, &inside);
    return ViewPix{*(const HPE_GAS unsigned short *)((const HPE_GAS char *)a.raw + off), i};
}
__device__ __forceinline__ float raw_value(const PrepArgsView &a, ViewPix p) {
    bool inside;
    (void)view_pick(a.view, p.i, &inside);
    return (float)(inside ? p.u : (unsigned short)0) * a.unit;
}

// The distance transform split over two launches (resident raw sequences; prep_dt_split).
// The frame a launch prepares has its forward scan in PrepArgs::dtf already; the scratch is
// double-buffered by frame parity.
struct PrepSplit {
    int *dtf_next;      // forward scan of the frame after the one prepared; null: no split
    int *r0, *r0_next;  // first hand row of the frame prepared / of the one after it
    int *seq_n;         // frames in the sequence (the call's prologue stores it)
};

// A lane's window (hpe_window, include/hpe.h: every bound inclusive) as the device table holds
// it, and the masking rule of the windowed preparation: pixel `pix` with raw value rv is kept iff
// its row, its column and its converted depth Z = to_cm ? (double)rv / 10. : (double)rv --
// prep_band's own expression -- lie inside; every other pixel reads as 0.0f.  Z is monotone in
// rv, so z_lo <= Z <= z_hi is raw_lo <= rv <= raw_hi for the smallest / largest float whose Z
// passes (win_raw_bounds, computed once when the entry is written, by the host or k_window_b):
// the same pixels exactly, without a fp64 division per pixel.  A select on a value already
// loaded: no load becomes conditional.  lo > hi or a NaN bound keeps nothing.
struct DevWindow {
    int row_lo, row_hi, col_lo, col_hi;
    double z_lo, z_hi;
    float raw_lo, raw_hi;  // z_lo, z_hi in the raw frame's unit (NaN: keeps nothing)
    int pad[2];
};
static_assert(sizeof(DevWindow) == 48, "a 16-byte multiple");
__host__ __device__ inline double win_depth(int to_cm, float rv) {
    return to_cm ? (double)rv / 10. : (double)rv;
}
// raw_lo = the smallest float f with win_depth(f) >= z_lo, raw_hi = the largest with
// win_depth(f) <= z_hi: the float nearest the bound in raw units, walked to the exact threshold
// (a step or two: the conversion is monotone, and -inf / +inf are floats like the others).
__host__ __device__ inline void win_raw_bounds(DevWindow &w, int to_cm) {
    const float inf = __builtin_inff();
    float lo = __builtin_nanf(""), hi = __builtin_nanf("");
    if (w.z_lo == w.z_lo) {
        lo = (float)(to_cm ? w.z_lo * 10.0 : w.z_lo);
        for (int k = 0; k < 8; ++k) {
            const float p = nextafterf(lo, -inf);
            if (p == lo || !(win_depth(to_cm, p) >= w.z_lo)) break;
            lo = p;
        }
        for (int k = 0; k < 8 && !(win_depth(to_cm, lo) >= w.z_lo); ++k) lo = nextafterf(lo, inf);
    }
    if (w.z_hi == w.z_hi) {
        hi = (float)(to_cm ? w.z_hi * 10.0 : w.z_hi);
        for (int k = 0; k < 8; ++k) {
            const float n = nextafterf(hi, inf);
            if (n == hi || !(win_depth(to_cm, n) <= w.z_hi)) break;
            hi = n;
        }
        for (int k = 0; k < 8 && !(win_depth(to_cm, hi) <= w.z_hi); ++k) hi = nextafterf(hi, -inf);
    }
    w.raw_lo = lo;
    w.raw_hi = hi;
}
__device__ __forceinline__ float win_raw(const DevWindow &w, int pix, float rv) {
    const int r = pix / HPE_IMG_W, c = pix - HPE_IMG_W * r;
    const bool keep = r >= w.row_lo && r <= w.row_hi && c >= w.col_lo && c <= w.col_hi &&
                      rv >= w.raw_lo && rv <= w.raw_hi;
    return keep ? rv : 0.0f;
}

// LDS layout: chunk[PREP_CH] doubles | acc1, flag (64 B) | wcnt, hcnt | mask bits | wmax
constexpr int prep_lds_bytes() {
    return PREP_CH * 8 + 64 + 2 * (PREP_NT / 64) * 4 + HPE_IMG_W * HPE_IMG_H / 32 * 4 + 64;
}

// inclusive prefix minimum over lanes 0..63 of a wave (DPP row shifts + row broadcasts)
__device__ __forceinline__ int wave_prefix_min(int v) {
    const int id = 0x7FFFFFFF;
    v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x118, 0xf, 0xf, false));  // row_shr:8
    v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    v = min(v, __builtin_amdgcn_update_dpp(id, v, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return v;
}
// inclusive prefix minimum of five values in two levels of v_min3
__device__ __forceinline__ void scan5_min(const int q[5], int p[5]) {
    p[0] = q[0];
    p[1] = min(q[0], q[1]);
    p[2] = min(min(q[0], q[1]), q[2]);
    p[3] = min(min(p[1], q[2]), q[3]);
    p[4] = min(min(p[2], q[3]), q[4]);
}
// value of lane l-1 (lane 0: fill) / lane l+1 (lane 63: fill)
__device__ __forceinline__ int from_left(int v, int fill) {
    return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xf, 0xf, false);  // wave_shr:1
}
__device__ __forceinline__ int from_right(int v, int fill) {
    return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xf, 0xf, false);  // wave_shl:1
}

// Producer side of a hand-off, then the arrival; returns (to every thread) whether this
// workgroup arrived last of `parties` (it then holds an agent acquire).
__device__ __forceinline__ bool prep_arrive_last(unsigned *ctr, unsigned parties, int *flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores are out
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned old = atomicAdd(ctr, 1u);
        const bool last = (old == parties - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            *ctr = 0u;  // ready for the next frame (the kernel boundary orders it)
        }
        *flag = last ? 1 : 0;
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(*flag) != 0;  // decides exits and barriers (§7)
}

// The same for many arriving workgroups: one counter per shard (blockIdx % ARRIVE_SHARDS,
// each on its own 128-B line) and a top counter the last of every shard increments, so
// no address takes more than parties / ARRIVE_SHARDS + ARRIVE_SHARDS atomics (hundreds of
// same-address atomics serialise at ~11-13 ns each).  ctr: ARRIVE_SHARDS * 32 + 1 words,
// reset by the last arriver.
#define ARRIVE_SHARDS 16
__device__ __forceinline__ bool arrive_last_sharded(unsigned *ctr, unsigned parties, int *flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned s = blockIdx.x % ARRIVE_SHARDS;
        const unsigned used = parties < ARRIVE_SHARDS ? parties : ARRIVE_SHARDS;
        const unsigned size = parties / ARRIVE_SHARDS + (s < parties % ARRIVE_SHARDS ? 1u : 0u);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bool last = false;
        if (atomicAdd(&ctr[s * 32], 1u) == size - 1) {  // last of its shard
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
            last = atomicAdd(&ctr[ARRIVE_SHARDS * 32], 1u) == used - 1;
        }
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            for (int k = 0; k < ARRIVE_SHARDS; ++k) ctr[k * 32] = 0u;  // for the next launch
            ctr[ARRIVE_SHARDS * 32] = 0u;
        }
        *flag = last ? 1 : 0;
    }
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(*flag) != 0;  // decides exits and barriers (§7)
}

// ---- band workgroup b: rows [30b, 30b + 30).  WIN: the raw values pass the lane's window *wn
// first (the batch calls' windowed kernels); the other forms compile as before.  A: PrepArgs, or
// PrepArgsU16 for 16-bit pixels -- the same pixel per thread per pass, so the same cloud order.
template <bool WIN = false, class A = PrepArgs>
__device__ __forceinline__ void prep_band(const A &a, int b, unsigned char *lds,
                                          const DevWindow *wn = nullptr) {
    constexpr int W = HPE_IMG_W, NWV = PREP_NT / 64;
    int *wcnt = (int *)(lds + PREP_CH * 8 + 64), *hcnt = wcnt + NWV;
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const double focal = a.focal;
    const double c0 = 320 / 2., c1 = 240 / 2.;
    const double Kv[9] = {focal, 0.0, c0, 0.0, focal, c1, 0.0, 0.0, 1.0};
    const int pbase = b * PREP_BAND_PIX;
    double *tmpb = a.tmp + 3 * (size_t)pbase, *ctbb = a.ctb + pbase;
    int base = 0, ncm = 0;
    if (t == 0) {  // after the DT workgroup's raw reads (bounded: ~1 ms, then go anyway)
        for (int i = 0; i < 4096 && __hip_atomic_load(&a.ctr[2], __ATOMIC_RELAXED,
                                                      __HIP_MEMORY_SCOPE_AGENT) == 0u; ++i)
            __builtin_amdgcn_s_sleep(8);
    }
    __syncthreads();
    // the band's raw pixels, all loads in flight at once (unconditional, clamped): one
    // round trip, also when the raw frame is read from pinned host memory over PCIe
    constexpr int NPASS = (PREP_BAND_PIX + PREP_NT - 1) / PREP_NT;
    decltype(raw_load(a, 0)) rvs[NPASS];
#pragma unroll
    for (int k = 0; k < NPASS; ++k) rvs[k] = raw_load(a, pbase + min(k * PREP_NT + t, PREP_BAND_PIX - 1));
#pragma unroll
    for (int k = 0; k < NPASS; ++k) {
        const int p0 = k * PREP_NT;
        const int q = p0 + t, pix = pbase + q;
        const bool in = q < PREP_BAND_PIX;
        const float rk = raw_value(a, rvs[k]);
        const float rv = WIN ? win_raw(*wn, pix, rk) : rk;
        const double Z = a.to_cm ? (double)rv / 10. : (double)rv;
        if (in) a.depth_cm[pix] = Z;
        const bool nz = in && Z != 0;
        const unsigned long long bm = __ballot(nz);
        const int wpre = __popcll(bm & ((1ull << l) - 1));
        double contrib = 0, X = 0, Y = 0;
        bool has = false;
        if (nz) {
            const int r = pix / W, c = pix - W * r;
            X = ((c - c0) * Z) / focal;
            Y = ((r - c1) * Z) / focal;
            const double ww = (Kv[6] * X + Kv[7] * Y) + Kv[8] * Z;
            const double u = (Kv[0] * X + Kv[1] * Y) + Kv[2] * Z;
            const double v = (Kv[3] * X + Kv[4] * Y) + Kv[5] * Z;
            const double Xe = X + 2.0;
            const double we = (Kv[6] * Xe + Kv[7] * Y) + Kv[8] * Z;
            const double ue = (Kv[0] * Xe + Kv[1] * Y) + Kv[2] * Z;
            const double ve = (Kv[3] * Xe + Kv[4] * Y) + Kv[5] * Z;
            const double du = floor(ue / we) - floor(u / ww);
            const double dv = floor(ve / we) - floor(v / ww);
            const double dn = sqrt(du * du + dv * dv);
            if (dn != 0) {
                contrib = 2.0 / dn;
                has = true;
            }
        }
        const unsigned long long bh = __ballot(has);
        const int hpre = __popcll(bh & ((1ull << l) - 1));
        if (l == 0) {
            wcnt[w] = __popcll(bm);
            hcnt[w] = __popcll(bh);
        }
        __syncthreads();
        int off = base, hoff = ncm, tot = 0, htot = 0;
#pragma unroll
        for (int k = 0; k < NWV; ++k) {
            off += (k < w) ? wcnt[k] : 0;
            hoff += (k < w) ? hcnt[k] : 0;
            tot += wcnt[k];
            htot += hcnt[k];
        }
        if (nz) {
            const int idx = off + wpre;
            tmpb[3 * idx + 0] = X;
            tmpb[3 * idx + 1] = Y * -1;
            tmpb[3 * idx + 2] = Z * -1;
        }
        if (has) ctbb[hoff + hpre] = contrib;  // the mean's terms, in pixel order
        base += tot;
        ncm += htot;
        __syncthreads();
    }
    if (t == 0) {
        a.info->band_n[b] = base;
        a.info->band_h[b] = ncm;
    }
}

// ---- merge (the last band to arrive): offsets, the scale mean, the (down-sampled) cloud
__device__ __forceinline__ void prep_merge(const PrepArgs &a, unsigned char *lds) {
    double *chunk = (double *)lds;
    double *acc1p = chunk + PREP_CH;
    const int t = threadIdx.x;
    int noff[PREP_BANDS + 1], hoff[PREP_BANDS + 1];
    noff[0] = hoff[0] = 0;
#pragma unroll
    for (int b = 0; b < PREP_BANDS; ++b) {
        noff[b + 1] = noff[b] + a.info->band_n[b];
        hoff[b + 1] = hoff[b] + a.info->band_h[b];
    }
    const int n_full = noff[PREP_BANDS], ncm = hoff[PREP_BANDS];
    // arma::mean = accumulate / n: two accumulators take the terms alternately, each a
    // sequential sum (arrayops::accumulate); threads 0 and 1 replay them from LDS chunks
    double acc = 0;
    for (int b0 = 0; b0 < ncm; b0 += PREP_CH) {
        const int m = min(PREP_CH, ncm - b0);
        for (int k = t; k < m; k += PREP_NT) {
            const int g = b0 + k;
            int b = 0;
#pragma unroll
            for (int q = 1; q < PREP_BANDS; ++q) b = (g >= hoff[q]) ? q : b;
            chunk[k] = a.ctb[(size_t)b * PREP_BAND_PIX + (g - hoff[b])];
        }
        __syncthreads();
        if (t < 2) {  // eight LDS reads in flight ahead of the dependent adds
            int k = ((b0 + t) & 1) ? 1 : 0;
            for (; k + 14 < m; k += 16) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = chunk[k + 2 * u];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
            }
            for (; k < m; k += 2) acc += chunk[k];
        }
        __syncthreads();
    }
    if (t == 1) *acc1p = acc;
    const int n = a.downsample ? 250 : n_full;
    const int f = n_full / 250;
    for (int k = t; k < n; k += PREP_NT) {
        double x = 0, y = 0, z = 0;
        const int src = a.downsample ? k * f : k;
        if (!a.downsample || n_full > 0) {
            int b = 0;
#pragma unroll
            for (int q = 1; q < PREP_BANDS; ++q) b = (src >= noff[q]) ? q : b;
            const double *p = a.tmp + 3 * ((size_t)b * PREP_BAND_PIX + (src - noff[b]));
            x = p[0];
            y = p[1];
            z = p[2];
        }
        a.cx[k] = x;
        a.cy[k] = y;
        a.cz[k] = z;
    }
    __syncthreads();
    if (t == 0) {
        a.info->n_full = n_full;
        a.info->n = n;
        a.info->scale = ncm ? (acc + *acc1p) / ncm : __builtin_nan("");
    }
}

// ---- DT workgroup: mask bits by all waves, the raster scans by wave 0.  WIN: the mask is of
// the raw values behind the lane's window *wn, the ones the bands read (A: as prep_band's).
template <bool WIN = false, class A = PrepArgs>
__device__ __forceinline__ void prep_dt(const A &a, unsigned char *lds,
                                        const DevWindow *wn = nullptr) {
    constexpr int W = HPE_IMG_W, H = HPE_IMG_H;
    unsigned *msk = (unsigned *)(lds + PREP_CH * 8 + 64 + 2 * (PREP_NT / 64) * 4);
    float *wmaxp = (float *)(msk + W * H / 32);
    const int t = threadIdx.x, l = t & 63;
    using raw_t = decltype(raw_load(a, 0));
#define DT_RAW_T raw_t
#define DT_RAW(i) raw_load(a, i)
#define DT_VAL(v) raw_value(a, v)
#define DT_HINT &a.ctr[2]
#define DT_FWD a.dtf
#define DT_OUT a.dt
#define DT_WIN(pix, v) (WIN ? win_raw(*wn, pix, v) : (v))
#define DT_PART 0
#include "hpe_dt_parts.inc"
    if (t < 64) {
#define DT_PART 1
#include "hpe_dt_parts.inc"
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#define DT_PART 2
#include "hpe_dt_parts.inc"
        if (l == 0) *wmaxp = mx;
    }
    __syncthreads();
    if (t == 0) a.info->dtmax = *wmaxp;
}
#undef DT_RAW_T
#undef DT_RAW
#undef DT_VAL
#undef DT_HINT
#undef DT_FWD
#undef DT_OUT
#undef DT_WIN

// ---- the transform split over two launches (resident raw sequences).  The
// backward scan starts where the forward scan ends, so one frame's transform cannot be
// shortened; but a launch can scan the frame it prepares backward, from forward values the
// PREVIOUS launch left, beside the forward scan of the frame after it for the NEXT launch:
// two independent half-transforms on two waves, the hand-off a kernel boundary.
// LDS words after the mask bits: [0] window / prep_dt's max, [1] first hand word, [2] the
// split transform's max (its own word: wave 0 may still read the window).

// Forward half by the whole workgroup: the mask of `raw` and its first hand row (all waves),
// then the forward scan by wave 0 into dtf and the row into *r0_out.
__device__ __forceinline__ void dt_forward_half(const float *raw, int *dtf, int *r0_out,
                                                unsigned char *lds) {
    constexpr int W = HPE_IMG_W, H = HPE_IMG_H;
    unsigned *msk = (unsigned *)(lds + PREP_CH * 8 + 64 + 2 * (PREP_NT / 64) * 4);
    const int t = threadIdx.x, l = t & 63;
#define DT_RAW_T float
#define DT_RAW(i) raw[i]
#define DT_VAL(v) (v)
#define DT_FWD dtf
#define DT_PART 0
#include "hpe_dt_parts.inc"
    if (t < 64) {
#define DT_PART 1
#include "hpe_dt_parts.inc"
        if (l == 0) *r0_out = r0;
    }
#undef DT_RAW_T
#undef DT_RAW
#undef DT_VAL
#undef DT_FWD
}

// The DT workgroup of a split preparation: wave 1 scans the frame being prepared backward
// from a.dtf / *ps.r0 into a.dt and dtmax; the workgroup runs the forward half of the frame
// after it (raw row *raw_row + 2) unless the sequence ends before it.
__device__ __forceinline__ void prep_dt_split(const PrepArgs &a, const PrepSplit &ps,
                                              unsigned char *lds) {
    constexpr int W = HPE_IMG_W, H = HPE_IMG_H;
    unsigned *msk = (unsigned *)(lds + PREP_CH * 8 + 64 + 2 * (PREP_NT / 64) * 4);
    float *wmaxp = (float *)(msk + W * H / 32 + 2);
    const int t = threadIdx.x, l = t & 63;
    // this workgroup reads another raw frame than the bands do: they need not wait for it
    if (t == 0) __hip_atomic_store(&a.ctr[2], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // decided from memory, and it decides barriers: uniform by readfirstlane
    const bool fwd = __builtin_amdgcn_readfirstlane(*a.raw_row + 2 < *ps.seq_n ? 1 : 0) != 0;
    // diagnostic build: the halves' spans from the workgroup's start, stamps 29 / 31 (100 MHz)
    const unsigned long long ts = HPE_STAMPS ? __builtin_amdgcn_s_memrealtime() : 0;
    auto span = [&](int k) {
        if (HPE_STAMPS && l == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            atomicAdd(&hpe_stamps[k], __builtin_amdgcn_s_memrealtime() - ts);
            atomicAdd(&hpe_stamps[32 + k], 1ull);
        }
    };
    // a.raw is raw row + 1 (prep_workgroup).  Every wave folds the mask (its barriers take the
    // whole workgroup, a few microseconds); then waves 0 and 1 scan side by side
    if (fwd) {
        dt_forward_half(a.raw + a.raw_stride, ps.dtf_next, ps.r0_next, lds);
        if (t < 64) span(29);
    }
    if ((t >> 6) == 1) {
        const int r0 = __builtin_amdgcn_readfirstlane(*ps.r0);
#define DT_FWD a.dtf
#define DT_OUT a.dt
#define DT_PART 2
#include "hpe_dt_parts.inc"
#undef DT_FWD
#undef DT_OUT
        if (l == 0) *wmaxp = mx;
        span(31);
    }
    __syncthreads();
    if (t == 0) a.info->dtmax = *wmaxp;
}

// The frame descriptor every tracking kernel reads.
__device__ __forceinline__ void prep_write_descriptor(const PrepArgs &a) {
    const PrepInfo *pi = a.info;
    DevObs od;
    od.cx = a.cx;
    od.cy = a.cy;
    od.cz = a.cz;
    od.depth = a.depth_cm;
    od.dt = a.dt;
    od.n = pi->n;
    od.lambda = (double)HPE_NS / (double)pi->n;  // costfunc.cpp:372
    od.scale = pi->scale;
    od.dtmax = pi->dtmax;
    const double Kv[9] = {a.focal, 0.0, 320 / 2., 0.0, a.focal, 240 / 2., 0.0, 0.0, 1.0};
    for (int k = 0; k < 9; ++k) od.K[k] = Kv[k];
    *a.obs_out = od;
}

// One preparing workgroup (index g in [0, PREP_WG)); the last to finish writes the
// descriptor.  With a split (ps and ps->dtf_next) the DT workgroup runs prep_dt_split.
// WIN: the bands and the transform's mask both read the frame through the window *wn (the
// split transform has no windowed form: the batch calls, which alone have windows, never split).
// A = PrepArgsU16: a frame of 16-bit pixels in a live batch's pinned ring, which has neither a
// raw row cursor nor a split; A = PrepArgsView: the same, a camera frame read through a view.
template <bool WIN = false, class A = PrepArgs>
__device__ __forceinline__ void prep_workgroup(const A &a0, int g, unsigned char *lds,
                                               const PrepSplit *ps = nullptr,
                                               const DevWindow *wn = nullptr) {
    constexpr bool U16 = std::is_base_of_v<PrepArgsU16, A>;
    int *flag = (int *)(lds + PREP_CH * 8 + 8);
    A a = a0;
    if (!U16 && a0.raw_row) a.raw = a0.raw + (size_t)(*a0.raw_row + 1) * a0.raw_stride;
    if (g < PREP_BANDS) {
        prep_band<WIN>(a, g, lds, wn);
        if (!prep_arrive_last(a.ctr, PREP_BANDS, flag)) return;
        prep_merge(a, lds);
    } else if (!WIN && !U16 && ps && ps->dtf_next) {
        prep_dt_split(a, *ps, lds);
    } else {
        prep_dt<WIN>(a, lds, wn);
    }
    if (prep_arrive_last(a.ctr + 1, 2, flag) && threadIdx.x == 0) {
        prep_write_descriptor(a);
        a.ctr[2] = 0u;  // every band is past its wait: ready for the next frame
    }
}

__global__ __launch_bounds__(PREP_NT) void k_prepare(PrepArgs a) {
    __shared__ __align__(16) unsigned char lds[prep_lds_bytes()];
    prep_workgroup(a, blockIdx.x, lds);
}

// Prologue of a resident raw sequence with the split transform, grid PREP_WG + 1: k_prepare's
// workgroups on frame 0 (a.raw), and one more that stores the sequence length n and, when
// there is a frame 1 (a.raw + a.raw_stride), its mask and forward scan for the first refine
// launch's backward half.
__global__ __launch_bounds__(PREP_NT) void k_prepare_seq(PrepArgs a, PrepSplit ps, int n) {
    __shared__ __align__(16) unsigned char lds[prep_lds_bytes()];
    if (blockIdx.x < PREP_WG) {
        prep_workgroup(a, blockIdx.x, lds);
        return;
    }
    if (threadIdx.x == 0) *ps.seq_n = n;
    if (n < 2) return;  // a kernel argument: uniform
    dt_forward_half(a.raw + a.raw_stride, ps.dtf_next, ps.r0_next, lds);
}

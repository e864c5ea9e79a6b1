// hpe_locate.hpp -- lane location (include/hpe.h "Lane location"): where the hand is in a raw
// depth frame, by the nearest-object rule, one workgroup per lane; and the placement of a
// caller's pose on the located centre, one wave per lane.  hpe/locate.py is the rule in numpy.
//
// k_locate_b reads the lane's raw frame in place three times (the histogram sweep and the two
// sum sweeps) rather than keeping each pixel's bin in LDS: a u16 bin per pixel is 150 KB, which
// with the 8 KB histogram and the reduction scratch only just fits a CU's 160 KB and leaves no
// room for a second workgroup; re-reading costs two more coalesced sweeps of 150-300 KB in a
// kernel that runs at initialisation and recovery, not per frame, and every sweep classifies a
// pixel by the same function (loc_pixel), so the three cannot disagree.  LDS: 8 KB histogram,
// 512 B of reduction scratch, a few broadcast words.
//
// Exactness: every count and sum is an integer (LDS atomics and shuffles: order-free), and every
// fp64 value is computed by thread 0 from those integers in the operation order the header
// writes, each operation a single IEEE one (the build's -ffp-contract=off; no product feeds an
// add anyway).  So the result equals the numpy mirror bit for bit.
#pragma once
#include "hpe_prep.hpp"
#include "hpe_report.hpp"

#define LOC_NT 1024
#define LOC_K 2048      // depth bins; bin LOC_K - 1 takes everything beyond
#define LOC_SLOT 128    // a lane's host slot: u64 begin | hpe_locate (104 bytes) | u64 end | pad
#define LOC_WORDS 13    // sizeof(hpe_locate) / 8
static_assert(sizeof(hpe_locate) == 8 * LOC_WORDS, "hpe_locate is 104 bytes");
static_assert(offsetof(hpe_locate, px) == 32 && offsetof(hpe_locate, centre) == 48 &&
              offsetof(hpe_locate, window) == 72, "hpe_locate's layout (include/hpe.h)");
static_assert(LOC_SLOT >= 8 * (LOC_WORDS + 2), "slot size");
static_assert(LOC_K == 2 * LOC_NT, "the scan gives every thread two bins");

// One lane's hpe_locate_params as the kernel takes it (sb = ceil(slab / bin), host-computed)
struct LocPar {
    int row_lo, row_hi, col_lo, col_hi;
    double z_lo, z_hi, bin, half_xy, half_z;
    int sb, skip, min_pixels, pad;
};
// A call's lanes, by value (as k_lane_act takes its words): each selected lane's raw frame --
// a live lane's pinned host buffer through its device pointer, or the context's staging
// buffer -- and its parameters
struct LocLanes {
    const void *raw[HPE_BATCH_MAX];
    LocPar par[HPE_BATCH_MAX];
};
// The templates of a placement call, by value: the caller's host array is read before the call
// returns, and no staging buffer has to outlive it
struct LocTmpl {
    double th[HPE_BATCH_MAX][HPE_DOF];
};
// The same with the lanes' views (a view batch's locate)
struct LocLanesView : LocLanes {
    hpe_view view[HPE_BATCH_MAX];
};
static_assert(sizeof(LocLanesView) <= 2048 && sizeof(LocTmpl) <= 3584, "kernel arguments");

struct LocBox {
    int row_lo, row_hi, col_lo, col_hi;
    double z_lo, z_hi;
};
// The hand box around pixel (r, c) at depth z: half_xy projected at z, each bound clamped in
// fp64 to the image and to the search window before its conversion to int (as the pose rule
// clamps), the depth bounds by comparisons (a NaN search bound keeps the box's own).
__device__ __forceinline__ LocBox loc_box(double r, double c, double z, double focal,
                                          const LocPar &p) {
    const double hx = (focal * p.half_xy) / z;
    LocBox b;
    b.row_lo = (int)fmin(fmax(ceil(r - hx), (double)max(0, p.row_lo)), (double)HPE_IMG_H);
    b.row_hi = (int)fmin(fmax(floor(r + hx), -1.0), (double)min(HPE_IMG_H - 1, p.row_hi));
    b.col_lo = (int)fmin(fmax(ceil(c - hx), (double)max(0, p.col_lo)), (double)HPE_IMG_W);
    b.col_hi = (int)fmin(fmax(floor(c + hx), -1.0), (double)min(HPE_IMG_W - 1, p.col_hi));
    double zl = z - p.half_z, zh = z + p.half_z;
    if (p.z_lo > zl) zl = p.z_lo;
    if (p.z_hi < zh) zh = p.z_hi;
    b.z_lo = zl;
    b.z_hi = zh;
    return b;
}

// Pixel `pix` of the lane's frame: its row, column, converted depth, whether it is valid (a
// finite positive raw value inside the search window: the masking rule's comparisons) and its
// depth bin -- one fp64 division, clamped in fp64 before the conversion.
struct LocPix {
    int r, c, k;
    double Z;
    bool valid;
};
// VIEW: raw is the lane's camera frame, and pixel `pix` of the model image is picked through the
// lane's view *vw (view_pick, hpe_prep.hpp: the preparation's own index arithmetic and select).
template <bool U16, bool VIEW = false>
__device__ __forceinline__ LocPix loc_pixel(const void *__restrict__ raw, int pix, float unit,
                                            int to_cm, const LocPar &p,
                                            const hpe_view *vw = nullptr) {
    static_assert(U16 || !VIEW, "a view reads 16-bit pixels");
    float rv;
    if constexpr (VIEW) {
        bool inside;
        const unsigned short u = ((const unsigned short *)raw)[view_pick(*vw, pix, &inside)];
        rv = (float)(inside ? u : (unsigned short)0) * unit;
    } else {
        rv = U16 ? (float)((const unsigned short *)raw)[pix] * unit : ((const float *)raw)[pix];
    }
    LocPix q;
    q.r = pix / HPE_IMG_W;
    q.c = pix - HPE_IMG_W * q.r;
    q.Z = win_depth(to_cm, rv);
    q.valid = isfinite(rv) && rv > 0.0f && q.r >= p.row_lo && q.r <= p.row_hi &&
              q.c >= p.col_lo && q.c <= p.col_hi && q.Z >= p.z_lo && q.Z <= p.z_hi;
    const double kf = floor(q.Z / p.bin);
    q.k = !q.valid ? 0 : kf >= (double)(LOC_K - 1) ? LOC_K - 1 : (int)kf;
    return q;
}

// {count, sum r, sum c, sum k} of the workgroup's selected pixels: wave shuffles, one LDS row
// per wave, then every thread adds the rows (all threads hold the totals).
struct LocSums {
    unsigned long long m, r, c, k;
};
__device__ __forceinline__ LocSums loc_block_sums(LocSums s, unsigned long long (*red)[4]) {
    for (int off = 32; off > 0; off >>= 1) {
        s.m += __shfl_xor(s.m, off);
        s.r += __shfl_xor(s.r, off);
        s.c += __shfl_xor(s.c, off);
        s.k += __shfl_xor(s.k, off);
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();  // the previous use of red is over
    if ((threadIdx.x & 63) == 0) {
        red[w][0] = s.m;
        red[w][1] = s.r;
        red[w][2] = s.c;
        red[w][3] = s.k;
    }
    __syncthreads();
    LocSums t{0, 0, 0, 0};
    for (int v = 0; v < LOC_NT / 64; ++v) {
        t.m += red[v][0];
        t.r += red[v][1];
        t.c += red[v][2];
        t.k += red[v][3];
    }
    return t;
}

// Grid B, one workgroup of LOC_NT threads per lane.  A lane outside `sel` clears its activity
// word and returns: it loads and stores nothing else.  A selected lane locates its frame; its
// thread 0 then writes the result record res[b], the activity word act[b] (HPE_ACT_PREP if
// found: the preparation and the placement that follow are gated by it, 0 if not) and, if found
// and wcur is non-null, the lane's window into wcur[b] (and woth[b], the other parity's table,
// under HPE_WINDOW_FIXED) with its depth bounds in raw units (win_raw_bounds).  host non-null:
// the record is also published to the lane's slot of the pinned host table with the report
// ring's begin / end words (hpe_report.hpp), seq = ++lane_seq[b] -- one thread stores the
// whole slot, every word a system-scope store, the end word a release.
// VIEW (hpe_batch_pipeline_begin_view): ln is a LocLanesView, the lanes' views behind the frames
// and parameters, and all three sweeps read the lane's camera frame through its view.
template <bool U16, bool VIEW = false>
__global__ __launch_bounds__(LOC_NT) void k_locate_b(std::conditional_t<VIEW, LocLanesView, LocLanes> ln,
                                                     unsigned sel, float unit, int to_cm,
                                                     double focal, DevWindow *__restrict__ wcur,
                                                     DevWindow *__restrict__ woth,
                                                     int *__restrict__ act,
                                                     hpe_locate *__restrict__ res,
                                                     unsigned long long *__restrict__ lane_seq,
                                                     unsigned long long *host) {
    constexpr int NPIX = HPE_IMG_H * HPE_IMG_W, NW = LOC_NT / 64;
    const int b = blockIdx.x, t = threadIdx.x, w = t >> 6, l = t & 63;
    if (!(sel >> b & 1)) {
        if (t == 0) act[b] = 0;
        return;
    }
    __shared__ unsigned hist[LOC_K];
    __shared__ unsigned long long red[NW][4];
    __shared__ unsigned wsum[NW];
    __shared__ int wmin[NW];
    __shared__ LocBox sbox;
    const void *__restrict__ const raw = ln.raw[b];
    const LocPar p = ln.par[b];
    hpe_view vw{};
    if constexpr (VIEW) vw = ln.view[b];

    // 1. the histogram of the valid pixels' bins, and the nearest bin past `skip` pixels
    hist[2 * t] = 0u;
    hist[2 * t + 1] = 0u;
    __syncthreads();
    for (int i = t; i < NPIX; i += LOC_NT) {
        const LocPix q = loc_pixel<U16, VIEW>(raw, i, unit, to_cm, p, &vw);
        if (q.valid) atomicAdd(&hist[q.k], 1u);
    }
    __syncthreads();
    const unsigned c0 = hist[2 * t], c1 = hist[2 * t + 1], own = c0 + c1;
    unsigned incl = own;  // inclusive scan over the wave, then the waves' totals
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned up = __shfl_up(incl, off);
        if (l >= off) incl += up;
    }
    if (l == 63) wsum[w] = incl;
    __syncthreads();
    unsigned before = incl - own;
    for (int v = 0; v < w; ++v) before += wsum[v];
    const unsigned skip = (unsigned)p.skip;  // >= 0 (the host checks); counts are <= 76800
    int cand = before + c0 > skip ? 2 * t : before + own > skip ? 2 * t + 1 : LOC_K;
    for (int off = 32; off > 0; off >>= 1) cand = min(cand, __shfl_xor(cand, off));
    if (l == 0) wmin[w] = cand;
    __syncthreads();
    int k_near = LOC_K;
    for (int v = 0; v < NW; ++v) k_near = min(k_near, wmin[v]);

    hpe_locate out{};
    out.lane = b;
    out.k_near = -1;
    if (k_near < LOC_K) {  // (workgroup-uniform: every thread holds the same k_near)
        out.k_near = k_near;
        // 2. pass 1: the slab behind the nearest bin
        const int k_hi = k_near + p.sb;  // sb <= LOC_K (the host clamps)
        LocSums s{0, 0, 0, 0};
        for (int i = t; i < NPIX; i += LOC_NT) {
            const LocPix q = loc_pixel<U16, VIEW>(raw, i, unit, to_cm, p, &vw);
            if (q.valid && q.k >= k_near && q.k <= k_hi) {
                s.m += 1;
                s.r += (unsigned)q.r;
                s.c += (unsigned)q.c;
                s.k += (unsigned)q.k;
            }
        }
        const LocSums s1 = loc_block_sums(s, red);
        out.m1 = (int)s1.m;  // > 0: bin k_near holds a pixel
        // 3. the box around the first centre
        if (t == 0) {
            const double r1 = (double)s1.r / (double)s1.m, c1d = (double)s1.c / (double)s1.m;
            const double z1 = ((double)s1.k / (double)s1.m + 0.5) * p.bin;
            sbox = loc_box(r1, c1d, z1, focal, p);
        }
        __syncthreads();
        const LocBox bx = sbox;
        // 4. pass 2: the valid pixels inside the box
        s = LocSums{0, 0, 0, 0};
        for (int i = t; i < NPIX; i += LOC_NT) {
            const LocPix q = loc_pixel<U16, VIEW>(raw, i, unit, to_cm, p, &vw);
            if (q.valid && q.r >= bx.row_lo && q.r <= bx.row_hi && q.c >= bx.col_lo &&
                q.c <= bx.col_hi && q.Z >= bx.z_lo && q.Z <= bx.z_hi) {
                s.m += 1;
                s.r += (unsigned)q.r;
                s.c += (unsigned)q.c;
                s.k += (unsigned)q.k;
            }
        }
        const LocSums s2 = loc_block_sums(s, red);
        out.m2 = (int)s2.m;
        if (s2.m > 0 && (long long)s2.m >= (long long)p.min_pixels) {
            // 5. the result, from the second centre
            const double r2 = (double)s2.r / (double)s2.m, c2 = (double)s2.c / (double)s2.m;
            const double z2 = ((double)s2.k / (double)s2.m + 0.5) * p.bin;
            const LocBox b2 = loc_box(r2, c2, z2, focal, p);
            out.found = 1;
            out.px[0] = c2;
            out.px[1] = r2;
            out.centre[0] = ((c2 - 160.0) * z2) / focal;
            out.centre[1] = ((r2 - 120.0) * z2) / focal;
            out.centre[2] = z2;
            out.window = hpe_window{b2.row_lo, b2.row_hi, b2.col_lo, b2.col_hi, b2.z_lo, b2.z_hi};
        }
    }
    if (t != 0) return;
    if (out.found && wcur) {
        DevWindow dw{out.window.row_lo, out.window.row_hi, out.window.col_lo, out.window.col_hi,
                     out.window.z_lo, out.window.z_hi, 0.f, 0.f, {0, 0}};
        win_raw_bounds(dw, to_cm);
        wcur[b] = dw;
        if (woth) woth[b] = dw;
    }
    act[b] = out.found ? HPE_ACT_PREP : 0;
    if (lane_seq) {
        out.seq = lane_seq[b] + 1;
        lane_seq[b] = out.seq;
    }
    res[b] = out;
    if (!host) return;
    typedef HPE_GAS unsigned long long gu64;
    gu64 *const slot = (gu64 *)host + (size_t)b * (LOC_SLOT / 8);
    unsigned long long words[LOC_WORDS];
    __builtin_memcpy(words, &out, sizeof(out));
    __hip_atomic_store(slot, out.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    for (int q = 0; q < LOC_WORDS; ++q)
        __hip_atomic_store(slot + 1 + q, words[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(slot + 1 + LOC_WORDS, out.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The placement rule, grid B, one wave per lane (sibling of k_window_b): a lane whose activity
// word lacks HPE_ACT_PREP -- unselected, or not found -- returns at entry and its row stays as
// it was.  FK of the lane's template under the lane's hand is fk_wave, as k_build runs it, so
// the centres are hpe_build_spheres' bit for bit; lane q < 3 sums coordinate q of the 48 centres
// in sphere order (y and z negated back), divides by 48 and stores theta 3 + q =
// T[3 + q] + (centre[q] - cen[q]); the other 23 entries are the template's.  The row's 27th
// entry is not written.
__global__ __launch_bounds__(64) void k_locate_place_b(LocTmpl tp, const DevHand *__restrict__ hands,
                                                       const hpe_locate *__restrict__ res,
                                                       const int *__restrict__ act,
                                                       double *__restrict__ states) {
    const int b = blockIdx.x, l = threadIdx.x;
    if (!(act[b] & HPE_ACT_PREP)) return;
    __shared__ DevHand hs;
    __shared__ FkSm fk;
    const double *__restrict__ const hw = (const double *)(hands + b);
    for (int q = l; q < (int)(sizeof(DevHand) / 8); q += 64) ((double *)&hs)[q] = gp(hw)[q];
    const double tv = tp.th[b][l < HPE_DOF ? l : HPE_DOF - 1];
    const double t3 = __shfl(tv, l < 3 ? 3 + l : l);  // lanes 0..2: T[3 + l]
    if (l < HPE_DOF) fk.th[l] = tv;
    __syncthreads();
    fk_wave(fk, &hs);
    __syncthreads();  // (one wave: the centres fk_wave's lanes stored, before other lanes read them)
    double *__restrict__ const row = states + (size_t)HPE_STATE_N * b;
    if (l < 3) {
        double acc = 0.0;
        for (int j = 0; j < HPE_NS; ++j) acc = acc + (l == 0 ? fk.S[j][l] : fk.S[j][l] * -1);
        const double cen = acc / (double)HPE_NS;
        row[3 + l] = t3 + (gp(res + b)->centre[l] - cen);
    }
    if (l < HPE_DOF && (l < 3 || l > 5)) row[l] = tv;
}

// hpe_clean.hpp -- lane cleaning (hpe_set_batch_clean, include/hpe.h "Lane cleaning"): the
// neighbourhood rule on a lane's 16-bit model image, ahead of the preparation.
//
// k_clean_b runs on grid (CLEAN_TILES, B): workgroup (g, b) cleans rows CLEAN_ROWS g ..
// CLEAN_ROWS g + 7 of lane b.  Thread t loads column t of the tile's ten rows -- its eight and
// one halo row above and below -- from the lane's source frame, each pixel of the frame once per
// workgroup that needs it and nothing else over the host link: the plain form reads src[320 r + t],
// the view form the camera pixel view_pick names (hpe_prep.hpp).  Every load is unconditional, from
// a row clamped into the image (and, through a view, view_pick's clamped index); a select zeroes
// what lay outside.  The rows go to LDS at a pitch of CLEAN_LP pixels with column c at index
// CLEAN_C0 + c, a zero at either end standing for columns -1 and 320.  After one barrier thread t
// takes the 3 x 10 patch around pixels 8 (t % 40) .. + 7 of tile row t / 40 into registers,
// applies the rule to its eight pixels and stores them as one 16-byte vector.
//
// No atomics, no flag, no hand-off between workgroups: every output depends on the source frame
// alone, and the destination is never the source.  act (free pacing; null: lockstep): a lane
// whose activity word lacks HPE_ACT_PREP has no next frame, and its workgroups return at entry.
#pragma once
#include "hpe_prep.hpp"

#define CLEAN_ROWS 8
#define CLEAN_NT HPE_IMG_W
#define CLEAN_TILES (HPE_IMG_H / CLEAN_ROWS)
#define CLEAN_C0 8
#define CLEAN_LP (HPE_IMG_W + 2 * CLEAN_C0)
static_assert(HPE_IMG_H % CLEAN_ROWS == 0 && HPE_IMG_W % 8 == 0 &&
                  CLEAN_ROWS * (HPE_IMG_W / 8) == CLEAN_NT,
              "one 8-pixel store per thread covers the tile");

// A lane's frames: what the kernel reads (a pinned buffer, or a staging copy of a host frame) and
// the 240x320 frame it writes.  Tables of these lie in device memory by [parity][lane], as the
// PrepArgs tables do: the graphs hold the table's address.
struct CleanArgs {
    const unsigned short *src;
    unsigned short *dst;
};
// The lanes' parameters (hpe_clean, 8 bytes each): device memory the host rewrites between calls.
struct CleanTab {
    hpe_clean par[HPE_BATCH_MAX];
};
static_assert(sizeof(hpe_clean) == 8, "hpe_clean is 8 bytes");

// The rule for one pixel: u, its eight neighbours n (0 outside the image), the lane's parameters.
__device__ __forceinline__ unsigned clean_pixel(unsigned u, const unsigned (&n)[8], int edge,
                                                int support, bool median) {
    bool nr[8];
    int s = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int d = (int)n[q] - (int)u;  // 32-bit: the values are depths up to 65535
        nr[q] = n[q] != 0u && (d < 0 ? -d : d) <= edge;
        s += nr[q] ? 1 : 0;
    }
    unsigned out = u;
    if (median) {  // (lane-uniform) the element of rank s / 2 of {u} and the near neighbours
        const int k = s >> 1;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const unsigned xj = j ? n[j - 1] : u;
            const bool vj = j ? nr[j - 1] : true;
            int lt = 0, le = 0;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const unsigned xi = i ? n[i - 1] : u;
                const bool vi = i ? nr[i - 1] : true;
                lt += (vi && xi < xj) ? 1 : 0;
                le += (vi && xi <= xj) ? 1 : 0;
            }
            out = (vj && lt <= k && k < le) ? xj : out;
        }
    }
    return (u != 0u && s >= support) ? out : 0u;
}

// vt: the batch's ViewTab (VIEW: lane b's source is its camera frame, picked through view[b]).
template <bool VIEW>
__global__ __launch_bounds__(CLEAN_NT) void k_clean_b(const CleanArgs *__restrict__ tab,
                                                      const CleanTab *__restrict__ ptab,
                                                      const ViewTab *__restrict__ vt,
                                                      const int *__restrict__ act) {
    const int b = blockIdx.y, t = threadIdx.x, r0 = CLEAN_ROWS * (int)blockIdx.x;
    if (act && !(act[b] & HPE_ACT_PREP)) return;
    __shared__ unsigned short tile[(CLEAN_ROWS + 2) * CLEAN_LP];
    const CleanArgs a = tab[b];
    const hpe_clean par = ptab->par[b];
    hpe_view vw{};
    if constexpr (VIEW) vw = vt->view[b];

    // 1. column t of the ten rows: ten independent loads, then the selects and the LDS stores
    unsigned short v[CLEAN_ROWS + 2];
    bool in[CLEAN_ROWS + 2];
#pragma unroll
    for (int k = 0; k < CLEAN_ROWS + 2; ++k) {
        const int r = r0 - 1 + k, rc = min(max(r, 0), HPE_IMG_H - 1);
        in[k] = (unsigned)r < (unsigned)HPE_IMG_H;
        int j = rc * HPE_IMG_W + t;
        if constexpr (VIEW) {
            bool inside;
            j = view_pick(vw, j, &inside);
            in[k] = in[k] && inside;
        }
        v[k] = *(const HPE_GAS unsigned short *)((const HPE_GAS char *)a.src + 2u * (unsigned)j);
    }
#pragma unroll
    for (int k = 0; k < CLEAN_ROWS + 2; ++k)
        tile[k * CLEAN_LP + CLEAN_C0 + t] = in[k] ? v[k] : (unsigned short)0;
    if (t < 2 * (CLEAN_ROWS + 2))  // columns -1 and 320
        tile[(t >> 1) * CLEAN_LP + ((t & 1) ? CLEAN_C0 + HPE_IMG_W : CLEAN_C0 - 1)] = 0;
    __syncthreads();

    // 2. eight pixels of one row
    const int row = t / (HPE_IMG_W / 8), c0 = 8 * (t - (HPE_IMG_W / 8) * row);
    unsigned w[3][10];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 10; ++i) w[k][i] = tile[(row + k) * CLEAN_LP + CLEAN_C0 - 1 + c0 + i];
    const bool median = (par.flags & HPE_CLEAN_MEDIAN) != 0;
    unsigned o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned n[8] = {w[0][i], w[0][i + 1], w[0][i + 2], w[1][i],
                               w[1][i + 2], w[2][i], w[2][i + 1], w[2][i + 2]};
        o[i] = clean_pixel(w[1][i + 1], n, (int)par.edge, (int)par.support, median);
    }
    // (a built-in vector: it stores through the address-space-1 pointer as one global store)
    typedef unsigned int CleanPack __attribute__((ext_vector_type(4)));
    const CleanPack pk = {o[0] | o[1] << 16, o[2] | o[3] << 16, o[4] | o[5] << 16, o[6] | o[7] << 16};
    *(HPE_GAS CleanPack *)((HPE_GAS unsigned short *)a.dst + (size_t)(r0 + row) * HPE_IMG_W + c0) = pk;
}

// hpe_dt_parts.inc -- the three pieces of the DT workgroup's chamfer transform (hpe_prep.hpp),
// included as text by the whole transform (prep_dt) and by the split one (dt_forward_half,
// prep_dt_split), so all compile the same statements.  DT_PART selects the piece; names expected
// in scope: W, H, msk, t, l and
//   0  mask + first hand row: DT_RAW(i) (the load of the raw frame's pixel i, of type DT_RAW_T)
//      and DT_VAL(v) (the raw float a loaded v stands for), optionally DT_HINT (word the band
//      workgroups wait for) and DT_WIN(pix, v) (the raw value v of pixel pix as the lane's
//      window leaves it); defines r0.  Every wave of the workgroup; two barriers.
//   1  forward scan by one wave: r0, DT_FWD (the forward values, written)
//   2  backward scan by one wave: r0, DT_FWD (read), DT_OUT (the float transform); defines mx,
//      the wave's largest distance
#if DT_PART == 0
    // hand = non-zero raw depth: 150 pixels per thread in three batches of 50 loads, the
    // next batch in flight while one is folded (unconditional: no branch splits them into
    // one round trip each; the raw frame may sit in pinned host memory, behind PCIe)
    constexpr int NPT = W * H / PREP_NT, B = NPT / 3;  // 150 pixels per thread, 3 batches
    static_assert(W * H % PREP_NT == 0 && NPT % 3 == 0, "whole batches");
    DT_RAW_T va[B], vb[B];
    auto issue = [&](DT_RAW_T (&v)[B], int k0) {
#pragma unroll
        for (int q = 0; q < B; ++q) v[q] = DT_RAW((k0 + q) * PREP_NT + t);
    };
    auto fold = [&](const DT_RAW_T (&v)[B], int k0) {
#pragma unroll
        for (int q = 0; q < B; ++q) {
            const int pix = (k0 + q) * PREP_NT + t;
#ifdef DT_WIN
            const unsigned long long bm = __ballot(DT_WIN(pix, DT_VAL(v[q])) != 0.f);
#else
            const unsigned long long bm = __ballot(DT_VAL(v[q]) != 0.f);
#endif
            if ((l & 31) == 0) msk[pix >> 5] = (unsigned)(bm >> (l & 32));
        }
    };
    issue(va, 0);
    issue(vb, B);
    fold(va, 0);
    issue(va, 2 * B);  // the third batch lands while the second is folded
    fold(vb, B);
    fold(va, 2 * B);
    // the band workgroups hold their own raw reads until here (a scheduling hint only):
    // when the frame sits in host memory the DT, the longer chain, gets PCIe to itself
#ifdef DT_HINT
    if (t == 0) __hip_atomic_store(DT_HINT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    int *rfirst = (int *)(msk + W * H / 32 + 1);
    if (t == 0) {
        msk[W * H / 32] = 0u;  // the two-word window of the last pixels
        *rfirst = 0x7FFFFFFF;
    }
    __syncthreads();
    for (int k = t; k < W * H / 32; k += PREP_NT) {  // first mask word holding a hand pixel
        if (msk[k] != 0u) {
            atomicMin(rfirst, k);
            break;
        }
    }
    __syncthreads();
    // The forward pass starts at the first row r0 holding a hand pixel.  Above it every
    // forward value is >= DT_INIT; with a hand pixel anywhere, every pixel's final value is
    // finite (< DT_INIT: a forward path right/down from some hand pixel, then a backward
    // path up/left, stays inside the image), so forward values >= DT_INIT never win a min
    // and any such value gives the same result: the rows above r0 start from DT_INIT, as
    // row 0 does, and the backward pass reads DT_INIT for them.  No hand pixel: r0 = 0.
    const int r0 = (*rfirst == 0x7FFFFFFF) ? 0 : *rfirst / (W / 32);
#elif DT_PART == 1
        // forward pass: lane l owns columns c0..c0+4; u1 / u2 = rows r-1 / r-2 at columns
        // c0-2 .. c0+6 (halo from the neighbour lanes)
        const int c0 = 5 * l;
        int u1[9], u2[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) u1[i] = u2[i] = DT_INIT;
        // rows in pairs from the even row at or above r0 (a row above r0 scanned from
        // DT_INIT is as good as unscanned, see above), two rows per trip
        static_assert(H % 2 == 0, "forward rows in pairs");
        auto row = [&](int r) {
            const int pix0 = r * W + c0;
            const unsigned long long mw =
                ((unsigned long long)msk[(pix0 >> 5) + 1] << 32) | msk[pix0 >> 5];
            const unsigned hb = (unsigned)(mw >> (pix0 & 31));
            int q[5], p[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int i = k + 2;
                // grouped by weight: min over the LONG, DIAG and HV neighbours, then the add
                const int mL = min(min(u2[i - 1], u2[i + 1]), min(u1[i - 2], u1[i + 2]));
                const int mD = min(u1[i - 1], u1[i + 1]);
                const int av = min(min(mL + DT_LONG, mD + DT_DIAG), u1[i] + DT_HV);
                // hand pixel -> 0: bit k sign-extended, then av & ~mask in one v_bfi
                const int m = __builtin_amdgcn_sbfe((int)hb, k, 1);
                q[k] = (av & ~m) - DT_HV * (c0 + k);
            }
            scan5_min(q, p);  // p[k] = min(q[0..k]), depth 2
            const int ex = from_left(wave_prefix_min(p[4]), 0x7FFFFFFF);  // lanes < l
            int T[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                // min(min(p, ex) + HV c, INIT + HV (c+1)) == min(p, ex, INIT + HV) + HV c
                T[k] = min(min(p[k], ex), DT_INIT + DT_HV) + DT_HV * (c0 + k);
                DT_FWD[pix0 + k] = T[k];
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) u2[i] = u1[i];
            u1[0] = from_left(T[3], DT_INIT);
            u1[1] = from_left(T[4], DT_INIT);
#pragma unroll
            for (int k = 0; k < 5; ++k) u1[k + 2] = T[k];
            u1[7] = from_right(T[0], DT_INIT);
            u1[8] = from_right(T[1], DT_INIT);
        };
        for (int r = r0 & ~1; r < H; r += 2) {
            row(r);
            row(r + 1);
        }
#elif DT_PART == 2
        // backward pass: lane l owns columns cb-k (cb = 319 - 5l, k = 0..4), i.e. scan
        // index j = 5l + k; d1 / d2 = rows r+1 / r+2 at scan positions j-2 .. j+6
        const int cb = W - 1 - 5 * l;
        int d1[9], d2[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) d1[i] = d2[i] = DT_INIT;
        float mx = 0.f;
        const float sc = 1.f / 65536;
        // forward values three rows ahead: row r's values are loaded while row r+3 is
        // scanned, into the register slot row r+3 just consumed (three slots, the loop
        // unrolled by three, so no register copy makes a row wait for newer loads);
        // unconditional loads of a clamped row
        int f0[5], f1[5], f2[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            f0[k] = DT_FWD[(H - 1) * W + cb - k];
            f1[k] = DT_FWD[(H - 2) * W + cb - k];
            f2[k] = DT_FWD[(H - 3) * W + cb - k];
        }
        auto step = [&](int r, int (&fs)[5]) {
            int fw[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) fw[k] = (r >= r0) ? fs[k] : DT_INIT;  // rows above r0: not scanned
            const int rn = r >= 3 ? r - 3 : 0;
#pragma unroll
            for (int k = 0; k < 5; ++k) fs[k] = DT_FWD[rn * W + cb - k];
            int q[5], p[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int i = k + 2;
                const int mL = min(min(d2[i - 1], d2[i + 1]), min(d1[i - 2], d1[i + 2]));
                const int mD = min(d1[i - 1], d1[i + 1]);
                const int bv = min(min(fw[k], mL + DT_LONG), min(mD + DT_DIAG, d1[i] + DT_HV));
                q[k] = bv - DT_HV * (5 * l + k);
            }
            scan5_min(q, p);
            const int ex = from_left(wave_prefix_min(p[4]), 0x7FFFFFFF);
            int T[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int j = 5 * l + k;
                T[k] = min(min(p[k], ex), DT_INIT + DT_HV) + DT_HV * j;
                const float v = (float)T[k] * sc;
                DT_OUT[r * W + cb - k] = v;
                mx = v > mx ? v : mx;
            }
#pragma unroll
            for (int i = 0; i < 9; ++i) d2[i] = d1[i];
            d1[0] = from_left(T[3], DT_INIT);
            d1[1] = from_left(T[4], DT_INIT);
#pragma unroll
            for (int k = 0; k < 5; ++k) d1[k + 2] = T[k];
            d1[7] = from_right(T[0], DT_INIT);
            d1[8] = from_right(T[1], DT_INIT);
        };
        static_assert(H % 3 == 0, "backward rows in threes");
        for (int r = H - 1; r >= 2; r -= 3) {
            step(r, f0);
            step(r - 1, f1);
            step(r - 2, f2);
        }
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(mx, off);
            mx = o > mx ? o : mx;
        }
#endif
#undef DT_PART

// hpe_window_body.inc -- the body of k_window_b (hpe_kernels.hip), text of its own as the other
// lane kernels' bodies are.  Names it expects in scope: HANDS (compile-time), states, Hg, par,
// wout (k_window_b's parameters).
    __shared__ DevHand hs;
    __shared__ FkSm fk;
    const int l = threadIdx.x;
    // the lane's hand: entry blockIdx.x of the table (this kernel's lane dimension is x)
    const double *__restrict__ const hw = (const double *)(HANDS ? Hg + blockIdx.x : Hg);
    for (int q = l; q < (int)(sizeof(DevHand) / 8); q += 64) ((double *)&hs)[q] = gp(hw)[q];
    if (l < HPE_DOF) fk.th[l] = states[(size_t)HPE_STATE_N * blockIdx.x + l];
    const WinPar p = *par;
    __syncthreads();
    window_wave(fk, &hs, p, wout + blockIdx.x);

// Persistent kernel, part 7: exit accounting of a launch without a tail (the last wave of the workgroup counts it out), and the -DPWV_PTRACE dump.
// Expects: parts 1, 2, tail_done.
    // The launch cleans up after itself: the LAST workgroup to finish zeroes every word a later launch polls (progress, abort,
    // this counter), so a launch that is handed this workspace again needs no zeroing kernel in front of it.  A wave counts
    // itself out only when its own global stores are complete (vmcnt(0)): no progress word can land after the zeroing.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (!tail_done) {
        int old = 0;
        if (lane == 0) old = __hip_atomic_fetch_add(&ctl[4], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (__builtin_amdgcn_readfirstlane(old) == 7) {
            int done = 0;
            if (lane == 0) done = __hip_atomic_fetch_add(p.exited, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__builtin_amdgcn_readfirstlane(done) == p.active_wgs - 1) {
                for (int k = lane; k < p.G * p.nwg; k += 64) __hip_atomic_store(p.prog + (size_t)k * kProgStride, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (SHORT) for (int k = lane; k < p.G * p.units; k += 64) __hip_atomic_store(p.uprog + (size_t)k * kUnitStride, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lane == 0) {
                    __hip_atomic_store(p.abort, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(p.exited, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
#ifdef PWV_PTRACE
    if (p.trace && lane == 0) {
        pt_acc[8] = __builtin_amdgcn_s_memtime();
        pt_acc[0] = pt_acc[8] - pt_start;
        long long* tr = p.trace + ((size_t)blockIdx.x * 8 + wave) * 24;
        for (int k = 0; k < 15; ++k) tr[k] = pt_acc[k];
        for (int k = 15; k < 18; ++k) tr[k + 6] = pt_acc[k];
        tr[16] = net; tr[17] = w; tr[18] = dead ? 1 : 0; tr[19] = __builtin_amdgcn_s_memrealtime(); tr[20] = pt_start_rt;
    }
#endif

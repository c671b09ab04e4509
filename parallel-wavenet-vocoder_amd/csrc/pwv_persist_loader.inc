// Persistent kernel, part 3: the loader wave of the short-input instantiation (wave 7).
// Expects: parts 1, 2.  Defines nothing.
    // ---- the loader (stationary units with an idle wave): it waits for the n active waves to have left layer jj, publishes the workgroup's
    // progress word and refills the LDS slot with layer jj + 2.  Left to the last wave to leave, as in the general scheme, the 80 KB of LDS-DMA
    // sit in THAT wave's memory queue in front of its next look-back row: 3 us on the top unit of every layer (r06_m timeline).
    if (loader_mode && wave == 7) {
        __builtin_amdgcn_s_setprio(0);      // (it shares its SIMD with an active wave)
        bool gone = false;
        for (int jj = 0; jj < L && !gone; ++jj) {
            const long long t0 = __builtin_amdgcn_s_memrealtime();
            for (int k = 0;; ++k) {
                if (__builtin_amdgcn_readfirstlane(*(__attribute__((address_space(3))) volatile int*)&ctl[8 + jj]) >= n) break;
                if (__builtin_amdgcn_readfirstlane(*(__attribute__((address_space(3))) volatile int*)&ctl[1])) { gone = true; break; }
                if ((k & 63) == 63 && (__builtin_amdgcn_readfirstlane(__hip_atomic_load(p.abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ||
                                       __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks)) {
                    __hip_atomic_store(p.status, 7, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    __hip_atomic_store(p.abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    *(__attribute__((address_space(3))) volatile int*)&ctl[1] = 1;
                    gone = true;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            if (gone) break;
            if (lane == 0) __hip_atomic_store(prog_n + (size_t)w * kProgStride, jj + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            PT_EV(7, jj, -1);
            if (jj + 2 < L) {
                fill_slot(jj & 1, jj + 2, 0, 1);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                lb[kWreadyB + (jj & 1)] = (unsigned char)(jj + 2);
            }
        }
    }

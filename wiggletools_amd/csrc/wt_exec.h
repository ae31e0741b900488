// wt_exec.h -- the vocabulary in which the five persistent kernels (wt_reduce_kernel.h, wt_patch_kernel.h, wt_delta_kernel.h,
// wt_walk_kernel.h) are written ONCE: hipcc compiles a body as the __global__ function it always was, g++ -DWT_EMU compiles the
// same text as an ordinary function template that drives one emulated workgroup (EmuRun R: tests/emu/wt_emu.cpp).  A body is the
// order of phase calls, the `if (tid ...)` guards, the chunk loops, the verdict branches and every barrier; the emulator queues
// what lies between two barriers and runs it at the barrier, wave by wave in the order the run asked for.
//
//                              device (hipcc)                                   emulator (-DWT_EMU)
//  WT_KERNEL(name, (b), a)     __global__ void __launch_bounds__(b) name(a)     void name(EmuRun &R, a)
//  WT_LDS(x)                   extern __shared__ ... char x[]                   char *x = R.lds.data()
//  WT_THREAD_IDS               const int tid = threadIdx.x, nt = blockDim.x     const int nt = R.plan.T  (tid: a fragment's argument)
//  WT_WG / WT_NWG              blockIdx.x / gridDim.x                           0 / 1  (one workgroup takes every ticket, every item;
//                                                                                its global slab is the one P.g_scratch points at)
//  WT_DO(v...) { ... } WT_END  { ... }                                          R.ph(nt, [&, v...](int tid) { ... });
//  WT_SYNC                     __syncthreads()                                  R.barrier()
//  WT_REG(x, type)             type x                                           std::vector<type> x(T)
//  WT_REG_INIT(x, v, type)     type x = v                                       std::vector<type> x(T, v)
//  WT_R(x)                     x                                                x[tid]
//  WT_EMU_ONLY(...)            nothing                                          ...  (the counters the tests read: n_redo, n_rounds, n_fallback)
//  WT_KERNEL_END               nothing                                          R.flush()  (fragments refer to the body's variables)
//  WT_MARK / WT_TICK / WT_PROF_BEGIN / WT_PROF_END: the -DWT_DEBUG_MARK / -DWT_PROFILE instrumentation; nothing in the emulator.
//
// WT_DO ... WT_END is a FRAGMENT: what every lane does next.  The emulator runs it at the next barrier, not where it stands, so
// every scalar of the body that the fragment reads and that changes or goes out of scope before that barrier (k, scale, ch,
// t_lo, ev0, ...) is listed and captured by value; everything else is seen by reference.  Statements outside a fragment run at
// once on both sides: uniform reads of LDS behind a barrier (the ticket, the verdicts, the window's run count).
// WT_REG is a lane register that lives across barriers; it is declared where the kernel declares it, inside or outside the
// window loop -- the lifetime is part of what the register allocator sees.
// A device call that is wave code (lane shuffles, ballots) has a substitute in the emulator; each is defined once, beside the
// device function it stands for (wt_delta.h: ranges, scans, escan; wt_walk.h: ranges; wt_walk_kernel.h:
// the stretch-walking rounds) or, the look-back's, below.  WT_SUBSYNC is the loop boundary inside such a substitute.
#ifndef WT_EXEC_H_
#define WT_EXEC_H_

#ifdef WT_EMU
#define WT_KERNEL(name, bounds, ...) void name(EmuRun &R, __VA_ARGS__)
#define WT_LDS(x) char *x = R.lds.data()
#define WT_THREAD_IDS const int nt = R.plan.T
#define WT_WG 0
#define WT_NWG 1
#define WT_DO(...) R.ph(nt, [& __VA_OPT__(,) __VA_ARGS__](int tid)
#define WT_END );
#define WT_SYNC R.barrier()
#define WT_SUBSYNC R.sub_barrier()
#define WT_REG(x, ...) std::vector<__VA_ARGS__> x(R.plan.T)
#define WT_REG_INIT(x, v, ...) std::vector<__VA_ARGS__> x(R.plan.T, v)
#define WT_R(x) x[tid]
#define WT_EMU_ONLY(...) __VA_ARGS__
#define WT_KERNEL_END R.flush()
#define WT_MARK(x) do { } while (0)
#define WT_TICK(slot) do { } while (0)
#define WT_PROF_BEGIN do { } while (0)
#define WT_PROF_END do { } while (0)
// The emulator's flavour of the look-back's wave code (wt_core.h: wt_lookback_publish / _complete, ballots), for one lane: publish is the same two stores; complete is the sequential walk over the predecessors'
// status words (wt_phase_lookback: windows run in ticket order there, so every predecessor has its inclusive prefix out and the
// walk is one step).
WT_DEV void wt_lookback_publish(const WtParams &P, WtCtx &c, long long k, unsigned long long mine) {
    c.sh->n_emit = (int32_t) mine;
    if (k > 0) wt_status_store(&P.status[k], WT_FLAG_AGG | mine);
}
WT_DEV void wt_lookback_publish(const WtParams &P, WtCtx &c, long long k) { wt_lookback_publish(P, c, k, (unsigned long long) c.epfx[P.n_words]); }
WT_DEV void wt_lookback_complete(const WtParams &P, WtCtx &c, long long k, int lane, unsigned long long mine) {
    if (lane == 0) wt_phase_lookback(P, c, k, mine);
}
WT_DEV void wt_lookback_complete(const WtParams &P, WtCtx &c, long long k, int lane) { wt_lookback_complete(P, c, k, lane, (unsigned long long) c.epfx[P.n_words]); }
#else
#define WT_KERNEL(name, bounds, ...) __global__ void __launch_bounds__ bounds name(__VA_ARGS__)
#define WT_LDS(x) extern __shared__ __attribute__((aligned(16))) char x[]
#define WT_THREAD_IDS const int tid = threadIdx.x, nt = blockDim.x
#define WT_WG blockIdx.x
#define WT_NWG gridDim.x
#define WT_DO(...)
#define WT_END
#define WT_SYNC __syncthreads()
#define WT_REG(x, ...) __VA_ARGS__ x
#define WT_REG_INIT(x, v, ...) __VA_ARGS__ x = v
#define WT_R(x) x
#define WT_EMU_ONLY(...)
#define WT_KERNEL_END do { } while (0)
// (WT_MARK reads k_dbg, WT_TICK prof / t_last: of the kernel that uses them)
#ifdef WT_MARK_ONLY
#define WT_MARK(x) do { if ((x) == WT_MARK_ONLY && (tid & 63) == 0) { P.debug[2 + (tid >> 6)] = (unsigned long long) (x); __threadfence_system(); } } while (0)
#elif defined(WT_DEBUG_MARK)
#define WT_MARK(x) do { if ((tid & 63) == 0) { if (tid == 0) { P.debug[0] = (unsigned long long) (x); P.debug[1] = (unsigned long long) k_dbg; } P.debug[2 + (tid >> 6)] = (unsigned long long) (x); __threadfence_system(); } } while (0)
#else
#define WT_MARK(x) do { } while (0)
#endif
#ifdef WT_PROFILE
// cycles of lane 0 between two ticks, by slot; added to P.counters[WT_CTR_PROF ..] when the workgroup ends
#define WT_TICK(slot) do { if (tid == 0) { const unsigned long long t_ = __builtin_readcyclecounter(); \
        prof[slot] += t_ - t_last; t_last = t_; } } while (0)
#define WT_PROF_BEGIN unsigned long long prof[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long t_last = __builtin_readcyclecounter()
#define WT_PROF_END do { if (tid == 0) for (int q = 0; q < 8; q++) wt_glb_add64(&P.counters[WT_CTR_PROF + q], prof[q]); } while (0)
#else
#define WT_TICK(slot) do { } while (0)
#define WT_PROF_BEGIN do { } while (0)
#define WT_PROF_END do { } while (0)
#endif
#endif

#endif  // WT_EXEC_H_

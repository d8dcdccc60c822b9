/*
 * ref_simt.h -- a CPU stand-in for the CUDA device environment, just large enough to execute
 * the reference's Chamfer and EMD kernels from their unmodified text (oracle/ref_build.py cuts
 * the kernels out of the reference checkout at build time; none of that text lives in this tree).
 *
 * TEST INFRASTRUCTURE ONLY, like the rest of oracle/.  Own code; single-threaded by design.
 *
 * Execution model
 *   - Blocks run one after another; inside a block, threads run ONE AT A TIME and switch only at
 *     __syncthreads() (each thread is a fiber on its own stack, with a guard page below it).  Nothing runs concurrently, so
 *     a launch is a pure function of its inputs and of the schedule.
 *   - Two schedules (ref_simt::Order): ASCENDING visits blocks (x fastest, then y, then z) and the
 *     threads of a block in increasing index order, DESCENDING visits both in decreasing order.
 *     Races of the real kernels ("last writer wins", non-atomic read-modify-write) resolve by that
 *     order; running a case under both tells whether it depends on the schedule at all.
 *   - A barrier releases when every thread of the block that has not yet returned has arrived
 *     (a thread that has returned no longer takes part).
 *   - __shared__ variables are function-local statics: one block is resident at a time.  Their
 *     contents survive from block to block like the stale contents of real shared memory; the
 *     kernels must not (and do not) read elements they have not written.
 *   - atomicAdd(float*) adds in schedule order.  When ref_simt::wide_begin() has registered a
 *     float buffer, every atomicAdd into it is ALSO accumulated in double precision in a shadow
 *     buffer: the float64 sum of the kernel's own fp32 terms, independent of any order.
 */
#ifndef GENPC_REF_SIMT_H
#define GENPC_REF_SIMT_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#if !defined(__x86_64__)
#error "ref_simt.h switches fibers with x86-64 System V assembly; the machines this project builds and tests on are x86-64"
#endif

struct uint3 { unsigned x, y, z; };
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {}
};

static uint3 threadIdx, blockIdx;
static dim3 blockDim, gridDim;

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static

namespace ref_simt {

enum Order { ASCENDING = 0, DESCENDING = 1 };

static const int MAX_THREADS = 1024;
static const size_t STACK_BYTES = 64 * 1024;
static const size_t GUARD_BYTES = 4096;

struct Fiber {
    void *sp;
    bool done;
};

static Fiber fibers[MAX_THREADS];
static char *stacks = nullptr;
static void (*body_call)(void *) = nullptr;
static void *body_ctx = nullptr;
static int current = -1;

/* One switch routine only: a Chamfer forward is 2 launches x 512 blocks x 512 threads x (1 + 2 per tile) switches,
 * millions per test case, and swapcontext() makes a system call (the signal mask) on each.
 * Saves the callee-saved registers of the System V ABI on the current stack, stores the stack
 * pointer through `save`, loads `load` and restores from there. */
extern "C" void ref_simt_switch(void **save, void *load);
asm(".text\n"
    ".p2align 4\n"
    ".local ref_simt_switch\n"
    ".type ref_simt_switch,@function\n"
    "ref_simt_switch:\n"
    "  pushq %rbp\n  pushq %rbx\n  pushq %r12\n  pushq %r13\n  pushq %r14\n  pushq %r15\n"
    "  movq %rsp, (%rdi)\n"
    "  movq %rsi, %rsp\n"
    "  popq %r15\n  popq %r14\n  popq %r13\n  popq %r12\n  popq %rbx\n  popq %rbp\n"
    "  ret\n"
    ".size ref_simt_switch,.-ref_simt_switch\n");
static void *sched_sp;
static inline void to_scheduler() { ref_simt_switch(&fibers[current].sp, sched_sp); }
static inline void to_fiber(int t) { ref_simt_switch(&sched_sp, fibers[t].sp); }

static void fiber_entry()
{
    body_call(body_ctx);
    fibers[current].done = true;
    to_scheduler();
    abort();                      /* a finished fiber is never resumed */
}

static void prepare(int t)
{
    char *top = stacks + (size_t)(t + 1) * STACK_BYTES;
    fibers[t].done = false;
    /* six saved registers, the entry as return address, one slot so that the entry sees the
     * stack alignment of an ordinary call */
    void **sp = (void **)top - 8;
    memset(sp, 0, 8 * sizeof(void *));
    sp[6] = (void *)fiber_entry;
    fibers[t].sp = sp;
}

static void run_block(int nthreads, Order order)
{
    for (int t = 0; t < nthreads; t++) prepare(t);
    int alive = nthreads;
    while (alive > 0) {
        /* one pass = every live thread runs up to its next barrier (or to its end) */
        for (int s = 0; s < nthreads; s++) {
            int t = order == ASCENDING ? s : nthreads - 1 - s;
            if (fibers[t].done) continue;
            current = t;
            threadIdx.x = (unsigned)t;
            to_fiber(t);
            if (fibers[t].done) alive--;
        }
    }
    current = -1;
}

template <class F> static void call_body(void *p) { (*(F *)p)(); }

/* grid.z and block.y / block.z are 1 in every launch of the reference; refuse anything else */
template <class F> static int launch(dim3 grid, dim3 block, Order order, F body)
{
    if (block.y != 1 || block.z != 1 || block.x < 1 || block.x > (unsigned)MAX_THREADS) return 0;
    if (grid.x < 1 || grid.y < 1 || grid.z != 1) return 0;
    if (!stacks) {
        void *p = mmap(nullptr, STACK_BYTES * MAX_THREADS, PROT_READ | PROT_WRITE,
                       MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (p == MAP_FAILED) return 0;
        stacks = (char *)p;
        /* the lowest page of every stack is a guard: a kernel that overflows its stack faults at once
         * instead of writing into its neighbour's */
        for (int t = 0; t < MAX_THREADS; t++)
            if (mprotect(stacks + (size_t)t * STACK_BYTES, GUARD_BYTES, PROT_NONE) != 0) return 0;
    }
    body_call = call_body<F>;
    body_ctx = &body;
    gridDim = grid;
    blockDim = block;
    threadIdx.y = threadIdx.z = 0;
    blockIdx.z = 0;
    unsigned nblocks = grid.x * grid.y;
    for (unsigned s = 0; s < nblocks; s++) {
        unsigned lin = order == ASCENDING ? s : nblocks - 1 - s;
        blockIdx.x = lin % grid.x;
        blockIdx.y = lin / grid.x;
        run_block((int)block.x, order);
    }
    return 1;
}

/* double-precision shadow of one float buffer (see the header comment) */
static float *wide_base[2];
static size_t wide_count[2];
static double *wide_sum[2];
static int wide_n = 0;

static inline void wide_begin(float *base, size_t count, double *sum)
{
    wide_base[wide_n] = base;
    wide_count[wide_n] = count;
    wide_sum[wide_n] = sum;
    wide_n++;
}
static inline void wide_end() { wide_n = 0; }

}  // namespace ref_simt

static inline void __syncthreads() { ref_simt::to_scheduler(); }

static inline int atomicAdd(int *address, int val)
{
    int old = *address;
    *address = old + val;
    return old;
}

static inline float atomicAdd(float *address, float val)
{
    float old = *address;
    *address = old + val;
    for (int w = 0; w < ref_simt::wide_n; w++) {
        if (address >= ref_simt::wide_base[w] && address < ref_simt::wide_base[w] + ref_simt::wide_count[w])
            ref_simt::wide_sum[w][address - ref_simt::wide_base[w]] += (double)val;
    }
    return old;
}

static inline int atomicCAS(int *address, int compare, int val)
{
    int old = *address;
    if (old == compare) *address = val;
    return old;
}

static inline int __float_as_int(float f) { int i; memcpy(&i, &f, sizeof i); return i; }
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, sizeof f); return f; }

/* CUDA's overloads of min / max in the forms the kernels use (float: fminf / fmaxf semantics) */
static inline int min(int a, int b) { return a < b ? a : b; }
static inline int max(int a, int b) { return a > b ? a : b; }
static inline float min(float a, float b) { return fminf(a, b); }
static inline float max(float a, float b) { return fmaxf(a, b); }

#endif

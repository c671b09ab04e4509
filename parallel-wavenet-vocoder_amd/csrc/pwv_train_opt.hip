// The optimiser of training over a gradient arena (include/pwv_hip_train_opt.h; DESIGN.md section 9, "Data-parallel training"): pack the
// gradients of a step into one flat buffer, unpack such a buffer into the tensors, and TensorFlow's Adam + the reference's EMA as one launch
// over the arenas.  Memory-bound: a capped grid of 256-lane workgroups loops over a host-built map of (tensor, chunk) records; a lane owns 4
// consecutive floats, 16 bytes per array.  One body (opt_walk) finds a lane's floats and hands them, as a quad or one by one, to the
// operation; no atomics, no LDS, padding floats of an arena are never written.
#include <cmath>

#include "pwv_common.h"
#include "pwv_hip_train_opt.h"

namespace pwv {

constexpr int kOptThreads = 256;
static_assert(kOptThreads * 4 == PWV_TRAIN_OPT_CHUNK, "a lane owns 4 floats of a chunk");

struct OptTables {
    const int64_t* table;               // [n][PWV_TRAIN_OPT_REC] = {address, offset, count}
    const int32_t* map;                 // [blocks][2] = {tensor, chunk}
    int blocks;
};

// The float32 constants of one Adam + EMA step, rounded once on the host (the header states the order of operations).
struct AdamConsts {
    float b1, c1, b2, c2, lr, eps, scale, d;
    int ema;
};

__device__ inline f32x4 load4(const float* p, bool vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(p);
    f32x4 r;
    r.x = p[0], r.y = p[1], r.z = p[2], r.w = p[3];
    return r;
}

__device__ inline void store4(float* p, f32x4 r, bool vec) {
    if (vec) {
        *reinterpret_cast<f32x4*>(p) = r;
    } else {
        p[0] = r.x, p[1] = r.y, p[2] = r.z, p[3] = r.w;
    }
}

// Every float of the launch once: op.quad(tensor + e, arena offset, tensor is 16-byte aligned) for 4 whole floats, op.one(tensor + e,
// arena offset) for each float of a tensor's tail.
template <class Op>
__device__ inline void opt_walk(const OptTables& t, Op op) {
    for (int b = blockIdx.x; b < t.blocks; b += gridDim.x) {
        const int i = t.map[2 * b], c = t.map[2 * b + 1];
        const int64_t* rec = t.table + (int64_t)i * PWV_TRAIN_OPT_REC;
        float* base = reinterpret_cast<float*>(rec[0]);
        const int64_t off = rec[1], count = rec[2];
        const int64_t e = (int64_t)c * PWV_TRAIN_OPT_CHUNK + 4 * (int64_t)threadIdx.x;
        if (e >= count) continue;
        if (e + 4 <= count) {
            op.quad(base + e, off + e, (rec[0] & 15) == 0);
        } else {
            for (int64_t k = e; k < count; ++k) op.one(base + k, off + k);
        }
    }
}

struct PackOp {
    float* arena;
    __device__ void quad(float* x, int64_t at, bool vec) const { *reinterpret_cast<f32x4*>(arena + at) = load4(x, vec); }
    __device__ void one(float* x, int64_t at) const { arena[at] = *x; }
};

struct UnpackOp {
    const float* arena;
    __device__ void quad(float* x, int64_t at, bool vec) const { store4(x, *reinterpret_cast<const f32x4*>(arena + at), vec); }
    __device__ void one(float* x, int64_t at) const { *x = arena[at]; }
};

// One rounding each, never fused with a neighbour.  (HIP's __fmul_rn / __fadd_rn are the plain operators inside header functions that
// are compiled with contraction allowed: once inlined, the compiler does fuse them into v_fma / v_pk_fma.  The operators below carry
// contract(off) themselves, which survives inlining.)
__device__ inline float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ inline float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ inline float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// One element of the step: exactly the operations of the header; the division is IEEE, sqrtf correctly rounded (hipcc's defaults).
__device__ inline void adam_ema_element(const AdamConsts& k, float grad, float& m, float& v, float& var, float& shadow) {
#pragma clang fp contract(off)
    const float g = mul_rn(k.scale, grad);
    m = add_rn(mul_rn(k.b1, m), mul_rn(k.c1, g));
    v = add_rn(mul_rn(k.b2, v), mul_rn(mul_rn(k.c2, g), g));
    var = sub_rn(var, mul_rn(k.lr, m) / add_rn(sqrtf(v), k.eps));
    if (k.ema) shadow = sub_rn(shadow, mul_rn(k.d, sub_rn(shadow, var)));
}

struct AdamOp {
    const float* grad;
    float* m;
    float* v;
    float* shadow;
    AdamConsts k;

    __device__ void quad(float* x, int64_t at, bool vec) const {
        const f32x4 g = *reinterpret_cast<const f32x4*>(grad + at);
        f32x4 m4 = *reinterpret_cast<const f32x4*>(m + at), v4 = *reinterpret_cast<const f32x4*>(v + at), x4 = load4(x, vec);
        f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
        if (k.ema) s4 = *reinterpret_cast<const f32x4*>(shadow + at);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float m1 = m4[j], v1 = v4[j], x1 = x4[j], s1 = s4[j];
            adam_ema_element(k, g[j], m1, v1, x1, s1);
            m4[j] = m1, v4[j] = v1, x4[j] = x1, s4[j] = s1;
        }
        *reinterpret_cast<f32x4*>(m + at) = m4;
        *reinterpret_cast<f32x4*>(v + at) = v4;
        store4(x, x4, vec);
        if (k.ema) *reinterpret_cast<f32x4*>(shadow + at) = s4;
    }

    __device__ void one(float* x, int64_t at) const {
        float m1 = m[at], v1 = v[at], x1 = *x, s1 = k.ema ? shadow[at] : 0.f;
        adam_ema_element(k, grad[at], m1, v1, x1, s1);
        m[at] = m1, v[at] = v1, *x = x1;
        if (k.ema) shadow[at] = s1;
    }
};

__global__ __launch_bounds__(kOptThreads) void opt_pack_kernel(OptTables t, PackOp op) { opt_walk(t, op); }
__global__ __launch_bounds__(kOptThreads) void opt_unpack_kernel(OptTables t, UnpackOp op) { opt_walk(t, op); }
__global__ __launch_bounds__(kOptThreads) void opt_adam_ema_kernel(OptTables t, AdamOp op) { opt_walk(t, op); }

// What every entry point refuses about its tables; all of it is read on the host.
static int opt_check_tables(const char* who, const int64_t* table, const int32_t* map, const int64_t* table_host, const int32_t* map_host,
                            int64_t arena_floats, int n, int blocks) {
    PWV_CHECK_ARG(table, "%s: table is a NULL pointer", who);
    PWV_CHECK_ARG(map, "%s: block_map is a NULL pointer", who);
    PWV_CHECK_ARG(table_host, "%s: table_host is a NULL pointer", who);
    PWV_CHECK_ARG(map_host, "%s: block_map_host is a NULL pointer", who);
    PWV_CHECK_ARG(n >= 1, "%s: n %d must be >= 1", who, n);
    PWV_CHECK_ARG(blocks >= 1, "%s: blocks %d must be >= 1", who, blocks);
    PWV_CHECK_ARG(arena_floats >= 1, "%s: arena_floats %lld must be >= 1", who, (long long)arena_floats);
    for (int i = 0; i < n; ++i) {
        const int64_t* r = table_host + (int64_t)i * PWV_TRAIN_OPT_REC;
        PWV_CHECK_ARG(r[0] != 0, "%s: table record %d: the tensor address is a NULL pointer", who, i);
        PWV_CHECK_ARG((r[0] & 3) == 0, "%s: table record %d: the tensor address %#llx is not 4-byte aligned", who, i, (unsigned long long)r[0]);
        PWV_CHECK_ARG(r[1] >= 0 && r[1] % 4 == 0, "%s: table record %d: offset %lld must be a multiple of 4 and >= 0", who, i, (long long)r[1]);
        PWV_CHECK_ARG(r[2] >= 1, "%s: table record %d: count %lld must be >= 1", who, i, (long long)r[2]);
        PWV_CHECK_ARG(r[1] <= arena_floats && r[2] <= arena_floats - r[1],
                      "%s: table record %d: offset %lld + count %lld overruns the arena (arena_floats %lld)", who, i, (long long)r[1],
                      (long long)r[2], (long long)arena_floats);
    }
    for (int b = 0; b < blocks; ++b) {
        const int i = map_host[2 * b], c = map_host[2 * b + 1];
        PWV_CHECK_ARG(i >= 0 && i < n, "%s: block_map record %d: tensor %d is outside 0 .. n - 1 = %d", who, b, i, n - 1);
        PWV_CHECK_ARG(c >= 0 && (int64_t)c * PWV_TRAIN_OPT_CHUNK < table_host[(int64_t)i * PWV_TRAIN_OPT_REC + 2],
                      "%s: block_map record %d: chunk %d begins behind the end of tensor %d (count %lld): it would overrun the arena", who, b, c,
                      i, (long long)table_host[(int64_t)i * PWV_TRAIN_OPT_REC + 2]);
    }
    return PWV_OK;
}

static int opt_check_arena(const char* who, const char* field, const void* p) {
    PWV_CHECK_ARG(p, "%s: %s is a NULL pointer", who, field);
    PWV_CHECK_ARG(((uintptr_t)p & 15) == 0, "%s: %s %p is not 16-byte aligned", who, field, p);
    return PWV_OK;
}

static unsigned opt_grid(int blocks) { return (unsigned)(blocks < PWV_TRAIN_OPT_MAX_GRID ? blocks : PWV_TRAIN_OPT_MAX_GRID); }

static int opt_copy(const pwv_train_opt_pack_args* a, const char* who, bool pack, hipStream_t st) {
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size == sizeof(pwv_train_opt_pack_args), "%s: struct_size %zu is not sizeof(pwv_train_opt_pack_args) = %zu", who,
                  a->struct_size, sizeof(pwv_train_opt_pack_args));
    if (int e = opt_check_arena(who, "arena", a->arena)) return e;
    if (int e = opt_check_tables(who, a->table, a->block_map, a->table_host, a->block_map_host, a->arena_floats, a->n, a->blocks)) return e;
    const OptTables t{a->table, a->block_map, a->blocks};
    if (pack)
        hipLaunchKernelGGL(opt_pack_kernel, dim3(opt_grid(a->blocks)), dim3(kOptThreads), 0, st, t, PackOp{a->arena});
    else
        hipLaunchKernelGGL(opt_unpack_kernel, dim3(opt_grid(a->blocks)), dim3(kOptThreads), 0, st, t, UnpackOp{a->arena});
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // namespace pwv

using namespace pwv;

extern "C" {

int pwv_train_opt_pack_f32(const pwv_train_opt_pack_args* a, pwv_stream_t stream) {
    return opt_copy(a, "pwv_train_opt_pack_f32", true, (hipStream_t)stream);
}

int pwv_train_opt_unpack_f32(const pwv_train_opt_pack_args* a, pwv_stream_t stream) {
    return opt_copy(a, "pwv_train_opt_unpack_f32", false, (hipStream_t)stream);
}

int pwv_train_opt_adam_ema_f32(const pwv_train_opt_adam_args* a, pwv_stream_t stream) {
    const char* who = "pwv_train_opt_adam_ema_f32";
    PWV_CHECK_ARG(a, "%s: args is NULL", who);
    PWV_CHECK_ARG(a->struct_size == sizeof(pwv_train_opt_adam_args), "%s: struct_size %zu is not sizeof(pwv_train_opt_adam_args) = %zu", who,
                  a->struct_size, sizeof(pwv_train_opt_adam_args));
    PWV_CHECK_ARG(std::isfinite(a->lr_t), "%s: lr_t %g must be finite", who, a->lr_t);
    PWV_CHECK_ARG(std::isfinite(a->grad_scale), "%s: grad_scale %g must be finite", who, a->grad_scale);
    PWV_CHECK_ARG(a->beta1 >= 0.0 && a->beta1 < 1.0, "%s: beta1 %g must be in [0, 1)", who, a->beta1);
    PWV_CHECK_ARG(a->beta2 >= 0.0 && a->beta2 < 1.0, "%s: beta2 %g must be in [0, 1)", who, a->beta2);
    PWV_CHECK_ARG(std::isfinite(a->eps) && a->eps >= 0.0, "%s: eps %g must be finite and >= 0", who, a->eps);
    PWV_CHECK_ARG(a->decay < 1.0, "%s: decay %g must be in [0, 1), or negative for no EMA", who, a->decay);
    const bool ema = a->decay >= 0.0;
    if (int e = opt_check_arena(who, "grad", a->grad)) return e;
    if (int e = opt_check_arena(who, "m", a->m)) return e;
    if (int e = opt_check_arena(who, "v", a->v)) return e;
    if (ema)
        if (int e = opt_check_arena(who, "shadow", a->shadow)) return e;
    if (int e = opt_check_tables(who, a->table, a->block_map, a->table_host, a->block_map_host, a->arena_floats, a->n, a->blocks)) return e;
    AdamConsts k;
    k.b1 = (float)a->beta1, k.c1 = (float)(1.0 - a->beta1), k.b2 = (float)a->beta2, k.c2 = (float)(1.0 - a->beta2);
    k.lr = (float)a->lr_t, k.eps = (float)a->eps, k.scale = (float)a->grad_scale;
    k.d = ema ? (float)(1.0 - a->decay) : 0.f, k.ema = ema ? 1 : 0;
    const OptTables t{a->table, a->block_map, a->blocks};
    hipLaunchKernelGGL(opt_adam_ema_kernel, dim3(opt_grid(a->blocks)), dim3(kOptThreads), 0, (hipStream_t)stream, t,
                       AdamOp{a->grad, a->m, a->v, ema ? a->shadow : nullptr, k});
    PWV_CHECK_HIP(hipGetLastError());
    return PWV_OK;
}

}  // extern "C"

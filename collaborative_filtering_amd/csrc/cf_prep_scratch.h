// cf_prep_scratch.h -- what the data-prep calls (cf_prep.hip, cf_split.hip) share beside the sorts
// of cf_sort.h: the context's prep scratch and its bump allocator, the events of cf_prep_timing and
// the capped grid of the element-wise kernels.  Everything has internal linkage.
#pragma once

#include "cf_internal.h"

namespace {

// the grid of an element-wise kernel over n entries: capped, so such a kernel strides
inline dim3 grid_for(uint64_t n) { return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 65536))); }

// Bump allocator over the context's prep scratch (grown to the request, 256 B aligned).
struct Carve {
    char* base;
    size_t used = 0;
    template <class T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(base + used);
        used += (sizeof(T) * std::max<size_t>(count, 1) + 255) & ~size_t(255);
        return p;
    }
};

inline int prep_reserve(cf_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->prep_bytes) return CF_OK;
    if (ctx->d_prep) (void)hipFree(ctx->d_prep);
    ctx->d_prep = nullptr;
    ctx->prep_bytes = 0;
    if (hipMalloc(&ctx->d_prep, bytes) != hipSuccess) return cf_set_error(ctx, CF_ENOMEM, "prep scratch");
    ctx->prep_bytes = bytes;
    return CF_OK;
}

inline int prep_events(cf_ctx* ctx) {
    for (hipEvent_t& e : ctx->prep_ev)
        if (!e) CF_HIP_CHECK(ctx, hipEventCreate(&e));
    return CF_OK;
}

}  // namespace

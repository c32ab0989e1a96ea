// Force-included ahead of cz_kernels.hip in a host-only compile (tools/dispatch_record.py): every
// hipLaunchKernelGGL prints the kernel as it is spelled, g(rid), b(lock), dynamic l(ds) bytes and every
// scalar or pointer argument instead of launching.  The kernel's address is never taken,
// so nothing of the device side has to link.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <type_traits>

namespace czrec {
template <class T>
void arg(const T &v)
{
    if constexpr (std::is_null_pointer_v<T>)
        std::printf(" null");
    else if constexpr (std::is_pointer_v<T>) {
        const uintptr_t p = (uintptr_t)v;  // the driver's made-up buffers: I(n), O(ut), K(eys), A(uxiliary) + offset
        if (p)
            std::printf(" %c+%llx", "?IOKA"[(p >> 40) < 5 ? p >> 40 : 0], (unsigned long long)(p & ((1ull << 40) - 1)));
        else
            std::printf(" null");
    } else if constexpr (std::is_integral_v<T> || std::is_enum_v<T>)
        std::printf(" %llu", (unsigned long long)v);
    else
        std::printf(" <%zu bytes>", sizeof(T));
}
template <class... A>
void launch(const char *kernel, dim3 grid, dim3 block, unsigned lds, const A &...a)
{
    std::printf("  %s g=%u b=%u l=%u :", kernel, grid.x, block.x, lds);
    (arg(a), ...);
    std::printf("\n");
}
}  // namespace czrec

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, grid, block, lds, s, ...) \
    czrec::launch(#k, dim3(grid), dim3(block), (unsigned)(lds), __VA_ARGS__)
// no device here: the launchers' own return values stay visible
#define hipGetLastError() hipSuccess

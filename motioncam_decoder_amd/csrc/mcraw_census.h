// mcraw_census.h -- what the path censuses share, for test builds only (DESIGN.md "The census layer").  A census is a counter
// array in device memory, an enum that names its counters, hooks in the kernels that are empty unless a test build's -D switch
// defines them, and an exported mcraw_diag_*_paths that reads the array; tests compare every counter with an exact model.  A
// family includes this header under its own switch (this header names none, so a variant compiles its family's sources alone)
// and brings the enum, the array and the hooks; here are the ways to count, the reader, and the list through which the sources
// of a family find each other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mcraw {

// ---- device side: `c` is the counter, &g_family_paths[slot]

// the active lanes for which `cond` holds (all active lanes of the wave call this together): a ballot, and the first active lane
// adds the population count
__device__ __forceinline__ void census_count(unsigned long long *c, bool cond)
{
    const unsigned long long m = __ballot(cond), act = __ballot(true);
    if (m != 0ull && (threadIdx.x & 63u) == static_cast<uint32_t>(__builtin_ctzll(act)))
        atomicAdd(c, static_cast<unsigned long long>(__popcll(m)));
}

// one for the wave (the lanes that are here) when `cond`, which is uniform over them, holds
__device__ __forceinline__ void census_wave(unsigned long long *c, bool cond)
{
    const unsigned long long act = __ballot(true);
    if (cond && (threadIdx.x & 63u) == static_cast<uint32_t>(__builtin_ctzll(act)))
        atomicAdd(c, 1ull);
}

// n for every lane for which `cond` holds
__device__ __forceinline__ void census_addn(unsigned long long *c, bool cond, uint32_t n)
{
    if (cond && n)
        atomicAdd(c, static_cast<unsigned long long>(n));
}

// one for the calling thread
__device__ __forceinline__ void census_one(unsigned long long *c) { atomicAdd(c, 1ull); }

// ---- host side

// The first N counters of `g` (an array may keep more behind them: `fold` brings those into the first N) into out[0 .. n), n
// clamped to N, in place of what is there or (`add`) on top of it; `reset`: and start the array over.  `out` may be null.
// Returns N.
template <int N, size_t TOTAL>
inline int census_read(unsigned long long (&g)[TOTAL], uint64_t *out, int n, int reset, bool add = false, void (*fold)(uint64_t *) = nullptr)
{
    static_assert(N <= static_cast<int>(TOTAL), "the family's counters are the array's first");
    (void)hipDeviceSynchronize();
    n = n < 0 ? 0 : n < N ? n : N;
    if (out && n) {
        uint64_t h[TOTAL];
        (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g), sizeof(h));
        if (fold)
            fold(h);
        for (int i = 0; i < n; i++)
            out[i] = (add ? out[i] : 0u) + h[i];
    }
    if (reset) {
        void *p = nullptr;
        (void)hipGetSymbolAddress(&p, HIP_SYMBOL(g));
        (void)hipMemset(p, 0, sizeof(g));
        (void)hipDeviceSynchronize(); // (the contexts' streams do not wait for the null stream)
    }
    return N;
}

// A family of several sources.  The library is linked without relocatable device code, so every source has a counter array of
// its own, of internal linkage; what the sources share is this list of their readers, one list per family (Family: the family's
// enum).  A source joins with one static CensusJoin<Family> object (the family's header defines it: including that header is
// joining), and census_sum adds up whoever joined.  The head is initialised at compile time, so the order in which the sources'
// objects are constructed when the library is loaded does not matter.
struct CensusSource {
    void (*read)(uint64_t *out, int n, int reset); // census_read of the source's array with `add`
    CensusSource *next;
};

template <class Family>
inline CensusSource *census_sources = nullptr;

template <class Family>
struct CensusJoin {
    CensusSource s;
    explicit CensusJoin(void (*read)(uint64_t *, int, int)) : s{read, census_sources<Family>} { census_sources<Family> = &s; }
};

template <class Family, int N>
inline int census_sum(uint64_t *out, int n, int reset)
{
    n = n < 0 ? 0 : n < N ? n : N;
    for (int i = 0; out && i < n; i++)
        out[i] = 0u;
    for (const CensusSource *s = census_sources<Family>; s && (out || reset); s = s->next)
        s->read(out, n, reset);
    return N;
}

} // namespace mcraw

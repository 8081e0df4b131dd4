// rt_record_stft_book.h -- host side of rt_fetch_record_stft (include/rt_analyze.h): the work list record_stft (rt_record_stft.h)
// runs from, and the one factor it multiplies by.  Host-only (no HIP): rt_analyze.hip calls it inside the entry, rt_hostcheck.cpp
// exports it to the CPU suite (hc_stft_*), tests/c/stft_work.cpp runs it under the sanitizers.
//
// A delivered call's snippets lie in its slot's pool in record order, whole segments only (rt_record_iq_book.h: iq_build_descs), so
// delivered segment g of the call -- counted over all records -- starts at sample g * N of the pool.  The kernel therefore needs no
// entry per segment: the records' first segments as a prefix [n + 1] (the IQ entry's offsets divided by N) and each record's bin
// are the whole list, and a wave finds its record by binary search over the prefix.
#ifndef RT_RECORD_STFT_BOOK_H
#define RT_RECORD_STFT_BOOK_H

#include <stdint.h>

#include <cmath>
#include <vector>

namespace rt {

struct StftWork {
    std::vector<int64_t> seg_first;  // [n + 1] delivered segments in front of each record; seg_first[n]: all of them
    std::vector<int32_t> fi;         // [n] each record's bin, fftfreq order
};

// `offsets` [n + 1]: IqSlot::offsets (samples); `fi` [n]: the records' bins.  Returns the call's delivered segments, or -1 where the
// lists are not what iq_build_descs writes (an offset that is no multiple of N or runs backwards, a bin outside 0 .. N - 1): the
// kernel indexes its twiddle table with fi and the pool with the prefix, so nothing is launched from such a list.
inline int64_t stft_build_work(const int64_t *offsets, const int32_t *fi, size_t n, int N, StftWork *w) {
    if (N < 1 || !offsets || offsets[0] != 0 || (n && !fi)) return -1;
    if (w) {
        w->seg_first.assign(n + 1, 0);
        w->fi.assign(n, 0);
    }
    for (size_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] % N != 0 || fi[i] < 0 || fi[i] >= N) return -1;
        if (w) {
            w->seg_first[i + 1] = offsets[i + 1] / N;
            w->fi[i] = fi[i];
        }
    }
    return offsets[n] / N;
}

// the record whose segments hold delivered segment g (0 <= g < seg_first[n]): the last one that starts at or before it -- records
// without a segment are stepped over.  The kernel's search, word for word.
inline int stft_record_of(const int64_t *seg_first, int n, int64_t g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_first[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// sqrt(scale), the factor between the windowed transform and a value: evaluated in float64, and on a float32 handle rounded once
inline float stft_root_f32(float scale) { return (float)std::sqrt((double)scale); }
inline double stft_root_f64(double scale) { return std::sqrt(scale); }

}  // namespace rt
#endif

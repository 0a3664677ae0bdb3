// segs_u64.hip -- sort_segs_tile<uint64_t> (the segment SORT tile of
// segs_tile.h; u64 and f64 keys), in its own translation unit so the key types
// compile in parallel.
#include "segs_tile.h"

namespace misort {
template hipError_t sort_segs_tile<uint64_t>(const uint64_t*, uint64_t*, const int64_t*, const uint32_t*, int64_t, int,
                                            int64_t, bool, hipStream_t, LaunchHook*);
}  // namespace misort

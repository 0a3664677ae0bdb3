// segs_u32.hip -- sort_segs_tile<uint32_t> (the segment SORT tile of
// segs_tile.h), in its own translation unit so the key types compile in parallel.
#include "segs_tile.h"

namespace misort {
template hipError_t sort_segs_tile<uint32_t>(const uint32_t*, uint32_t*, const int64_t*, const uint32_t*, int64_t, int,
                                            int64_t, bool, hipStream_t, LaunchHook*);
}  // namespace misort

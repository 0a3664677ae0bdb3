// rows_u32.hip -- sort_rows_tile<uint32_t> (the row-wise SORT tile of
// rows_tile.h), in its own translation unit so the key types compile in parallel.
#include "rows_tile.h"

namespace misort {
template hipError_t sort_rows_tile<uint32_t>(const uint32_t*, uint32_t*, int64_t, int64_t, bool, hipStream_t,
                                            LaunchHook*);
}  // namespace misort

// rows_u64.hip -- sort_rows_tile<uint64_t> (the row-wise SORT tile of
// rows_tile.h; u64 and f64 keys), in its own translation unit so the key types
// compile in parallel.
#include "rows_tile.h"

namespace misort {
template hipError_t sort_rows_tile<uint64_t>(const uint64_t*, uint64_t*, int64_t, int64_t, bool, hipStream_t,
                                            LaunchHook*);
}  // namespace misort

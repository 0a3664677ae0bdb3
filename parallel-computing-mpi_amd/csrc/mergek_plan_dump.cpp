// mergek_plan_dump.cpp -- prints what mergek_plan.h decides, as one JSON line
// (host compiler only; tests/test_runsk_model.py reads the shipped numbers here):
//   mergek_plan_dump key_bytes lk fence_log2              the chunk shape's constants
//   mergek_plan_dump n lw lk key_bytes fence_log2 [depth] the PassPlan, layout included
//                                                         (n[,n...]: one line per n)
// It reads the same MISORT_* knobs from its environment as the library.  Exit
// status 2 on arguments merge_levelk would reject.  mergek_plan_dump_impl.h (the
// plan header and the printing) is compiled once per fence stride, each in its
// own namespace, as runsk.hip is.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

namespace fg7 {
#define MISORT_RUNSK_FGL 7
#include "mergek_plan_dump_impl.h"
#undef MISORT_RUNSK_FGL
}  // namespace fg7
namespace fg6 {
#define MISORT_RUNSK_FGL 6
#include "mergek_plan_dump_impl.h"
#undef MISORT_RUNSK_FGL
}  // namespace fg6

int main(int argc, char** argv) {
    if (argc < 4 || argc > 7 || argc == 5) {
        fprintf(stderr, "usage: %s key_bytes lk fence_log2 | n lw lk key_bytes fence_log2 [depth]\n", argv[0]);
        return 2;
    }
    const int fgl = atoi(argv[argc == 4 ? 3 : 5]);
    if (fgl != 6 && fgl != 7) return 2;
    return fgl == 6 ? fg6::dump(argc, argv) : fg7::dump(argc, argv);
}

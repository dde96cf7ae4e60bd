// csrc/enabled_state.h on its own (no HIP header, no library): an extraction after a culled scan keeps the mirror and
// leaves both sets of block popcounts; borrowing the scratch costs the directory and nothing else.
#include <stdio.h>

#include "enabled_state.h"

int main()
{
    rh_enabled_state s;
    int bad = 0;
    s.bits_replaced(true); s.directory_built(); s.list_built();
    bad += !(s.has_directory() && s.has_list() && s.has_mirror());
    s.scratch_taken(); s.scan_started(true, true);
    bad += !(!s.has_directory() && s.has_mirror() && s.scan_left_sums());
    s.scan_folded(true); s.directory_built();
    bad += !(s.has_mirror() && !s.has_block_sums() && !s.has_list() && !s.long_window(true) && s.long_window(true));
    printf("%d bad\n", bad);
    return bad != 0;
}

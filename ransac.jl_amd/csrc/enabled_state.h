// enabled_state.h -- which structures derived from rh_cloud::enabled still match the bits.  Host only, no HIP.  Callers
// report events and ask queries; DESIGN.md §3, "The enabled bits and what follows them", says what each event invalidates.
#pragma once

class rh_enabled_state {
public:
    // ---- events: the bits changed
    void bits_replaced(bool mirror_copied) { bits_changed(); k_men_valid = mirror_copied; }
    void bits_cleared_by_list(bool mirror_updated) { bits_changed(); if (!mirror_updated) k_men_valid = false; }
    void scan_folded(bool has_blocks)   // enabled &= ~refit_mask; has_blocks: the new bits' block popcounts are left
    {
        const bool mirror_kept = k_applied && k_men_valid;   // (only a scan that ran ahead in the mirror keeps it)
        k_applied = false;
        bits_changed();
        k_men_valid = mirror_kept;
        en_sums_valid = has_blocks;
    }
    // ---- events: the bits did not change
    // (a culled scan with `apply` runs ahead in the mirror and leaves refit_mask's block popcounts in the scan scratch)
    void scan_started(bool culled, bool apply) { scan_dropped(); k_applied = k_sums_ready = culled && apply; }
    void scratch_taken() { select_valid = false; k_sums_ready = false; }
    void directory_built() { select_valid = true; sel_valid = crec_valid = en_sums_valid = false; very_long_windows = 0; }
    void list_built() { sel_valid = select_valid; }
    void records_built() { crec_valid = has_list(); }
    void mirror_built() { k_men_valid = true; k_applied = false; }
    // a long sampling window (very_long: 8 x longer) reads the list; true: give it the compact records (from the second very long one on)
    bool long_window(bool very_long)
    {
        if (very_long && very_long_windows < 2) very_long_windows++;
        return has_records() || (very_long && very_long_windows >= 2);
    }
    // ---- queries
    bool has_directory() const { return select_valid; }               // word_prefix, and d_total is its total
    bool has_list() const { return select_valid && sel_valid; }       // sel_list
    bool has_records() const { return select_valid && crec_valid; }   // crec
    bool has_mirror() const { return k_men_valid; }                   // oct_men
    bool has_block_sums() const { return en_sums_valid; }             // en_block_sums: the directory skips its popcount pass
    bool scan_left_sums() const { return k_sums_ready; }              // block_sums: the fold skips its popcount pass
    int long_windows() const { return very_long_windows; }

private:
    void scan_dropped() { if (k_applied) k_men_valid = false; k_applied = k_sums_ready = false; }   // (ahead, never folded)
    void bits_changed() { scan_dropped(); select_valid = en_sums_valid = false; }
    bool select_valid = false, sel_valid = false, crec_valid = false, en_sums_valid = false, k_men_valid = false, k_applied = false, k_sums_ready = false;
    int very_long_windows = 0;
};

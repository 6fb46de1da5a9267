// TEST-ONLY driver of csrc/sph_carry.hpp (what each entry point drops of the state a step leaves behind) on the CPU: for every case it
// sets every flag valid and the mover word nonzero, applies the row (or the rows an entry point composes) and prints what remains;
// tests/test_carry_host.py compares cell by cell.  Built with plain g++ under AddressSanitizer + UBSan; no HIP.
//
//   <case> hdr_ahead=0|1 ahead_valid=.. grid_valid=.. export_valid=.. prob_open=.. slab_lists_valid=.. slab_rows_open=.. have_level=..
//          have_reduced=.. lists_after=.. inc_count_valid=.. movers_word=.. have_flags=.. rnd_have_prev=..
#include <cstdio>
#include <initializer_list>

#include "sph_carry.hpp"

static volatile uint32_t g_word;   // stands in for the mapped mover-count word

static Carry all_valid(bool with_word = true)
{
    Carry c;
    c.hdr_ahead = c.ahead_valid = c.grid_valid = c.export_valid = c.prob_open = c.slab_lists_valid = c.slab_rows_open = true;
    c.have_level = c.have_reduced = c.lists_after = c.inc_count_valid = c.have_flags = c.rnd_have_prev = true;
    g_word = 7u;
    c.movers_host = with_word ? &g_word : nullptr;
    return c;
}

static void print(const char* name, const Carry& c)
{
    printf("%s hdr_ahead=%d ahead_valid=%d grid_valid=%d export_valid=%d prob_open=%d slab_lists_valid=%d slab_rows_open=%d have_level=%d "
           "have_reduced=%d lists_after=%d inc_count_valid=%d movers_word=%d have_flags=%d rnd_have_prev=%d\n",
           name, c.hdr_ahead, c.ahead_valid, c.grid_valid, c.export_valid, c.prob_open, c.slab_lists_valid, c.slab_rows_open, c.have_level,
           c.have_reduced, c.lists_after, c.inc_count_valid, g_word != 0u, c.have_flags, c.rnd_have_prev);
}

static void sequence(const char* name, std::initializer_list<unsigned> rows, bool with_word = true)
{
    Carry c = all_valid(with_word);
    for (unsigned r : rows) c.drop(r);
    print(name, c);
}

int main()
{
    // ---- the named rows
    sequence("classify", {DROPS_CLASSIFY});
    sequence("field_position", {drops_upload_field(CARRY_F_POSITION)});
    sequence("field_mass", {drops_upload_field(CARRY_F_MASS)});
    sequence("field_particle_id", {drops_upload_field(CARRY_F_PARTICLE_ID)});
    sequence("field_other", {drops_upload_field(2)});   // (velocity)
    sequence("transfer", {DROPS_TRANSFER});
    sequence("deletion", {DROPS_DELETION});
    sequence("regather", {DROPS_REGATHER});
    sequence("export_early", {DROPS_EXPORT_EARLY});
    sequence("edits_early", {DROPS_EDITS_EARLY});
    sequence("upload", {DROPS_UPLOAD});
    sequence("policy", {DROPS_POLICY});
    sequence("dist_configure", {DROPS_DIST_CONFIGURE});
    sequence("step_start", {DROPS_STEP_START});
    sequence("step_failed", {DROPS_STEP_FAILED});
    sequence("nothing", {0u});
    // ---- what the entry points compose
    sequence("share", {DROPS_TRANSFER});
    sequence("merge_no_deletion", {DROPS_EXPORT_EARLY, DROPS_TRANSFER});
    sequence("merge_deletion", {DROPS_EXPORT_EARLY, DROPS_TRANSFER, DROPS_DELETION, DROPS_REGATHER});
    sequence("split_nobody", {DROPS_EXPORT_EARLY});
    sequence("split", {DROPS_EXPORT_EARLY, DROPS_REGATHER});
    sequence("edits", {DROPS_EDITS_EARLY, DROPS_REGATHER});
    // ---- no mapped word yet: the flag goes, nothing is written
    sequence("upload_without_word", {DROPS_UPLOAD}, false);
    // ---- the open problem: a re-export of the valid CSR keeps it, a rebuild closes it
    {
        Carry c = all_valid();
        c.export_built();
        print("reexport_valid", c);
        c.drop(CARRY_EXPORT);
        c.export_built();
        print("rebuild", c);
        c.prob_open = true;   // (opened on the new CSR)
        c.export_built();
        print("reopened_reexport", c);
    }
    return 0;
}

// TEST INFRASTRUCTURE ONLY: the span check of the between-step layers' entry points (wheeledlab_amd/csrc/wl_layer_common.h: overlap, Span,
// any_overlap) compiled for the host through the stand-in hip_runtime.h, as a stand-alone program on hand-made cases -- and the place for
// a -fsanitize=address,undefined run of that code.  Every span lies inside one buffer of 64 bytes (or is NULL); nothing is dereferenced.
//
//   layer_spans_host        prints one line per case: "<name> <0 | 1>", what any_overlap says; tests/test_layers_cpu.py holds what it must say
#include <hip/hip_runtime.h>

#include <cstdio>

#include "wl_layer_common.h"

int main() {
    static unsigned char buf[64];
    const unsigned char* b = buf;
    int shown = 0;
    const auto show = [&](const char* name, bool got) {
        std::printf("%s %d\n", name, got ? 1 : 0);
        ++shown;
    };
    {   // a stored span and two read spans, far apart
        const Span v[] = {{b, 8}, {b + 16, 8}, {b + 40, 8}};
        show("disjoint", any_overlap(v, 1));
    }
    {   // the read span begins at the byte after the stored span's last, and the other ends at the byte before its first
        const Span v[] = {{b + 8, 8}, {b + 16, 8}, {b, 8}};
        show("touching_end_to_start", any_overlap(v, 1));
    }
    {   // the read span's first byte is the stored span's last
        const Span v[] = {{b, 8}, {b + 7, 8}};
        show("one_byte_stored_then_read", any_overlap(v, 1));
    }
    {   // the read span's last byte is the stored span's first
        const Span v[] = {{b + 7, 8}, {b, 8}};
        show("one_byte_read_then_stored", any_overlap(v, 1));
    }
    {   // an absent optional argument overlaps nothing, whatever its length says; as a stored span too
        const Span v[] = {{b, 16}, {nullptr, 64}, {b + 16, 4}};
        show("null_read_span", any_overlap(v, 1));
        const Span w[] = {{nullptr, 64}, {b, 16}, {b + 8, 4}};
        show("null_stored_span", any_overlap(w, 1));
    }
    {   // the second stored span lies on the LAST read span: every stored span is held against every later span
        const Span v[] = {{b, 8}, {b + 8, 8}, {b + 16, 4}, {b + 20, 4}, {b + 12, 16}};
        show("stored_on_a_later_read_span", any_overlap(v, 2));
    }
    {   // two stored spans on each other
        const Span v[] = {{b, 8}, {b + 4, 8}, {b + 32, 4}};
        show("stored_on_stored", any_overlap(v, 2));
    }
    {   // two read spans on each other (the same flags twice, a state row read by two terms): allowed
        const Span v[] = {{b, 8}, {b + 16, 8}, {b + 16, 8}, {b + 20, 8}};
        show("read_on_read", any_overlap(v, 1));
    }
    {   // the corruption entry point's table: a fixed array whose unused entries are NULL spans, a used one far down it
        Span v[8] = {{b, 8}, {nullptr, 0}, {b + 8, 8}};
        show("null_tail", any_overlap(v, 2));
        v[7] = Span{b + 4, 8};
        show("used_entry_behind_null_ones", any_overlap(v, 2));
    }
    {   // one span inside another; a span of one byte at either end
        const Span v[] = {{b, 32}, {b + 8, 4}};
        show("contained", any_overlap(v, 1));
        const Span w[] = {{b + 8, 4}, {b + 7, 1}, {b + 12, 1}};
        show("single_bytes_outside", any_overlap(w, 1));
        const Span x[] = {{b + 8, 4}, {b + 11, 1}};
        show("single_byte_inside", any_overlap(x, 1));
    }
    return shown == 14 ? 0 : 1;
}

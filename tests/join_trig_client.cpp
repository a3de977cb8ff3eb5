// Host build of csrc/dd_trig.h for tests/test_join_ref_cpu.py: reads doubles (hex floats, one per line; four per line after the
// word "dot"), prints sincos_rn's s and c, or dot2_rn's value, as hex floats.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../slam.jl_amd/csrc/dd_trig.h"

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        if (!strncmp(line, "dot", 3)) {
            char* p = line + 3;
            double v[4];
            for (int i = 0; i < 4; ++i) v[i] = strtod(p, &p);
            printf("%a\n", dot2_rn(v[0], v[1], v[2], v[3]));
            continue;
        }
        double s, c;
        sincos_rn(strtod(line, nullptr), &s, &c);
        printf("%a %a\n", s, c);
    }
    return 0;
}

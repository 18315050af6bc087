// Stand-alone probe of csrc/env.h for tests/test_env_cpu.py (host compiler, no HIP).
//   env_probe read   NAME DFLT       -> env_once(NAME, DFLT)
//   env_probe once   NAME DFLT NEW   -> env_once before and after setenv(NAME, NEW) in this process
//   env_probe switch NAME DFLT NEW   -> env_switch before and after the same setenv
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "env.h"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const char* name = argv[2];
    const long dflt = atol(argv[3]);
    if (!strcmp(argv[1], "read")) {
        printf("%ld\n", skimi::env_once(name, dflt));
        return 0;
    }
    if (argc < 5) return 2;
    const bool once = !strcmp(argv[1], "once");
    const long first = once ? skimi::env_once(name, dflt) : skimi::env_switch(name, dflt);
    setenv(name, argv[4], 1);
    const long second = once ? skimi::env_once(name, dflt) : skimi::env_switch(name, dflt);
    printf("%ld %ld\n", first, second);
    return 0;
}

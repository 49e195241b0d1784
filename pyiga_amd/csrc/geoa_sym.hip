// k_geoA instantiations with the pair-product sweep (symmetric fixed forms, P <= 5): geoa.hip compiled a second time for these
// alone, with the code-generator option that keeps the rotating pair window a lattice of wave-uniform jumps (Makefile:
// GEOA_SYM_FLAGS).  Everything else of geoa.hip -- the other instantiations, the tables, the launches -- lives in geoa.o.
#define GEOA_SYM_TU
#include "geoa.hip"

// Host program of tests/test_grid_choice.py: prints what pcg128.h decides
// about the masking launch's grid, for comparison with Python integers.
//   "cf <g> <0|1>"          carry_free of the tile jump of a g-block grid
//   "qg <cap> <tiles> <g>"  qualifying_grid(tiles, cap)
#include <stdio.h>

#include "../../sfl_amd/csrc/pcg128.h"

int main() {
  for (int g = 1; g <= 2048; g++)
    printf("cf %d %d\n", g, (int)sa::carry_free(sa::jump_of((uint64_t)g * sa::kTile - (sa::kE - 1)).mult));
  const int caps[] = {256, 496, 511, 512, 1792};
  for (int cap : caps)
    for (int t = 1; t <= 2048; t++) printf("qg %d %d %d\n", cap, t, sa::qualifying_grid((uint64_t)t, cap));
  return 0;
}

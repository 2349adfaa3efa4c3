// The failure counter and the check of the stand-alone test programs: a failed
// EXPECT is reported with its place and counted; each program prints the count
// in its summary line and returns it as (part of) its exit status.
#pragma once
#include <stdio.h>

static int fails = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                        \
    }                                                                 \
  } while (0)

// args_check.h -- what the stand-alone *_args_check.cpp programs of this directory share: the status comparison, the
// host buffers that stand in for device pointers, and the final report.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define EXPECT(expr, want) do { int got_ = (expr); if (got_ != (want)) { ++fails; std::printf("line %d: got %d want %d\n", __LINE__, got_, (want)); } } while (0)

// `slots` buffers of `slot` bytes each, one after the other, the first 256-byte aligned: arena(i) is buffer i
struct Arena {
  size_t slot;
  std::vector<char> raw;
  char* base;
  Arena(size_t slot, int slots) : slot(slot), raw(slot * slots + 256), base((char*)(((uintptr_t)raw.data() + 255) / 256 * 256)) {}
  char* operator()(int i) const { return base + slot * i; }
};

// the last line of every program, and main's return value
static int report() {
  std::printf("%s: %d failures\n", fails ? "FAILED" : "ok", fails);
  return fails != 0;
}

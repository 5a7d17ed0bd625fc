/* Test-only: what every stand-alone sanitizer program (tests/take, tests/append, tests/batch: *_san_main.c) had of its own: the
 * check that ends the program, and a small generator. A program that draws from it sets rnd_state to its own seed first thing in
 * main, so each keeps its own sequence. */
#ifndef SAN_UTIL_H
#define SAN_UTIL_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static uint32_t rnd_state;
static inline uint32_t rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
#endif

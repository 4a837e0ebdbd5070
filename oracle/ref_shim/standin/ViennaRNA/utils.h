/* Stand-in for <ViennaRNA/utils.h> (test infrastructure only): the one
 * function the reference's loader factory names.  The shims never call it. */
#ifndef SKREF_STANDIN_VIENNARNA_UTILS_H
#define SKREF_STANDIN_VIENNARNA_UTILS_H
static inline void init_rand(void) {}
#endif

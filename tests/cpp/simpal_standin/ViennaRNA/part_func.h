/* Stand-in for <ViennaRNA/part_func.h> (test infrastructure only): empty, the
 * harness supplies PFWrapper::fold itself. */

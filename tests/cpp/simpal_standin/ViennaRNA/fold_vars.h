/* Stand-in for <ViennaRNA/fold_vars.h> (test infrastructure only): the
 * reference's PFWrapper names only this type. */
#ifndef SK_SIMPAL_STANDIN_FOLD_VARS_H
#define SK_SIMPAL_STANDIN_FOLD_VARS_H
typedef double FLT_OR_DBL;
#endif

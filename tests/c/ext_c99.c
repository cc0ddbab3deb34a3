/* C99 consumer of include/ndfft_mi355x_ext.h: the header compiles under -std=c99 -pedantic -Werror, the entry point links, and a call
 * without a plan is refused with NDFFT_ERR_INVALID_ARG (needs no GPU). */
#include <stdio.h>
#include <string.h>

#include "ndfft_mi355x_ext.h"

typedef int (*weighted_fn)(const ndfft_plan *, int, const void *, void *, int, const int64_t *, const int64_t *, const int64_t *, const int64_t *, int,
                           const void *, size_t, void *);

int main(void) {
    weighted_fn f = ndfft_exec_weighted_device;
    int64_t shape[1] = {4}, stride[1] = {1};
    if (ndfft_abi_minor() < 4) { printf("abi minor %d\n", ndfft_abi_minor()); return 1; }
    if (f(NULL, NDFFT_OP_C2C_INV, NULL, NULL, 1, shape, stride, shape, stride, 0, NULL, 4, NULL) != NDFFT_ERR_INVALID_ARG) { printf("null plan accepted\n"); return 1; }
    if (strcmp(ndfft_last_error(), "plan is null") != 0) { printf("message: %s\n", ndfft_last_error()); return 1; }
    printf("ext c99 ok\n");
    return 0;
}

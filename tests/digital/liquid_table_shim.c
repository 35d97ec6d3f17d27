/*
 * liquid_table_shim.c -- TEST INFRASTRUCTURE ONLY.  Compiled by tests/table_oracle.py at test time and linked against the oracle's loader
 * of the reference liquid-dsp 1.5.0 binary; the product never sees it.
 *
 * What the table-driven constellations need beyond liquid_digital_shim.c (whose modemcf wrappers serve every modem object, these included):
 * a SysV wrapper around the ms_abi export modemcf_create_arbitrary, and a reader of the binary's APSK descriptions, which it exports as
 * data (liquid_apsk4 .. liquid_apsk256).  Nothing of those descriptions is stored anywhere: the tests compare them, at test time, with what
 * csdr_design_rings derives from the modulator's points.
 */
#include <stdint.h>
#include <string.h>

#define MS __attribute__((ms_abi))

int liquid_ref_load(const char *path);
void *pe_sym(const char *name);

typedef void *(MS *modem_create_arb_t)(const float *, unsigned int);

/* struct liquid_apsk_s of the 64-bit binary */
struct apsk_def {
    int scheme;
    unsigned int num_levels;
    unsigned int *p;
    float *r;
    float *phi;
    float *r_slicer;
    unsigned char *map;
};

static void *sym(const char *name)
{
    if (liquid_ref_load(NULL)) return 0;
    return pe_sym(name);
}

int shim_table_ready(void)
{
    return sym("modemcf_create_arbitrary") && sym("liquid_apsk4") && sym("liquid_apsk8") && sym("liquid_apsk16") && sym("liquid_apsk32") &&
           sym("liquid_apsk64") && sym("liquid_apsk128") && sym("liquid_apsk256");
}

/* modemcf_create_arbitrary(table, M): n interleaved complex points (the object rescales them: read its points back through the modulator) */
void *shim_modem_create_arbitrary(const float *points, int n)
{
    return ((modem_create_arb_t)sym("modemcf_create_arbitrary"))(points, (unsigned int)n);
}

/* the binary's description of APSK-M: returns num_levels (0: no such export); p / r / phi hold num_levels entries, slicer num_levels - 1,
 * map M (symbol -> ring-ordered index); each array has room for 8 resp. 256 entries */
int shim_apsk_read(int M, unsigned int *p, float *r, float *phi, float *slicer, unsigned char *map)
{
    const char *name = M == 4 ? "liquid_apsk4" : M == 8 ? "liquid_apsk8" : M == 16 ? "liquid_apsk16" : M == 32 ? "liquid_apsk32" :
                       M == 64 ? "liquid_apsk64" : M == 128 ? "liquid_apsk128" : M == 256 ? "liquid_apsk256" : 0;
    const struct apsk_def *d = name ? (const struct apsk_def *)sym(name) : 0;
    if (!d || d->num_levels < 1 || d->num_levels > 8) return 0;
    const unsigned int L = d->num_levels;
    memcpy(p, d->p, L * sizeof(unsigned int));
    memcpy(r, d->r, L * sizeof(float));
    memcpy(phi, d->phi, L * sizeof(float));
    memcpy(slicer, d->r_slicer, (L - 1) * sizeof(float));
    memcpy(map, d->map, (size_t)M);
    return (int)L;
}

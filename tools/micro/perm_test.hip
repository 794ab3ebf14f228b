// micro test: v_perm_b32 byte selectors on gfx950 as the flag planes of k_align16p.hip use them - 0..7 pick a byte of {src0 : src1} (src1 = bytes 0..3),
// 8..11 give 0xFF / 0x00 by the sign of bits 15, 31, 47, 63 of {src0 : src1}
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
__global__ void k(const uint32_t* a, const uint32_t* b, uint32_t* out) {
    const int i = threadIdx.x;
    uint32_t d0, d1, d2;
    asm volatile("v_perm_b32 %0, %1, %2, %3" : "=v"(d0) : "v"(a[i]), "v"(b[i]), "s"(0x0B0A0908));
    asm volatile("v_perm_b32 %0, %1, %2, %3" : "=v"(d1) : "v"(a[i]), "v"(b[i]), "s"(0x06040200));
    asm volatile("v_perm_b32 %0, %1, %2, %3" : "=v"(d2) : "v"(a[i]), "v"(b[i]), "s"(0x07050301));
    out[3 * i] = d0; out[3 * i + 1] = d1; out[3 * i + 2] = d2;
}
static uint32_t model(uint32_t a, uint32_t b, uint32_t sel) {
    const uint64_t in = ((uint64_t)a << 32) | b; uint32_t r = 0;
    for (int k = 0; k < 4; ++k) {
        const int s = (sel >> (8 * k)) & 0xff; uint32_t byte;
        if (s < 8) byte = (uint32_t)(in >> (8 * s)) & 0xff;
        else if (s < 12) byte = ((in >> (16 * (s - 8) + 15)) & 1) ? 0xff : 0;
        else byte = s == 12 ? 0 : 0xff;
        r |= byte << (8 * k);
    }
    return r;
}
int main() {
    const int N = 256; uint32_t ha[N], hb[N], ho[3 * N]; uint32_t x = 12345;
    for (int i = 0; i < N; ++i) { x = x * 1664525u + 1013904223u; ha[i] = x; x = x * 1664525u + 1013904223u; hb[i] = x; }
    ha[0] = 0; hb[0] = 0; ha[1] = 0xffffffffu; hb[1] = 0xffffffffu; ha[2] = 0x80000000u; hb[2] = 0x00008000u; ha[3] = 0x00008000u; hb[3] = 0x80000000u;
    uint32_t *da, *db, *dout;
    if (hipMalloc(&da, sizeof ha) || hipMalloc(&db, sizeof hb) || hipMalloc(&dout, sizeof ho)) { printf("alloc failed\n"); return 2; }
    if (hipMemcpy(da, ha, sizeof ha, hipMemcpyHostToDevice) || hipMemcpy(db, hb, sizeof hb, hipMemcpyHostToDevice)) { printf("copy failed\n"); return 2; }
    k<<<1, N>>>(da, db, dout);
    if (hipMemcpy(ho, dout, sizeof ho, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 2; }
    const uint32_t sels[3] = {0x0B0A0908u, 0x06040200u, 0x07050301u}; int bad = 0;
    for (int i = 0; i < N; ++i) for (int s = 0; s < 3; ++s) {
        const uint32_t e = model(ha[i], hb[i], sels[s]);
        if (ho[3 * i + s] != e && bad++ < 8) printf("a %08x b %08x sel %08x: got %08x exp %08x\n", ha[i], hb[i], sels[s], ho[3 * i + s], e);
    }
    printf(bad ? "PERM MISMATCH\n" : "PERM OK\n");
    return bad ? 1 : 0;
}

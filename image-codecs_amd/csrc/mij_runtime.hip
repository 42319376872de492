/*
 * mij_runtime.hip -- host side of the C-ABI in include/mij.h: contexts, batches (pinned staging,
 * device arenas, one HIP stream each), upload / launch / fetch, measurement hooks.
 * The kernels are in mij_kernels.h.  No exceptions and no C++ types cross the ABI.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "mij.h"
#include "mij_host.h"
#include "mij_internal.h"
#include "mij_kernels.h"
#include "mij_scaled_kernels.h"
#include "mij_entropy_kernels.h"
#include "mij_planes_out_kernels.h"
#include "mij_libjpeg_kernels.h"

using namespace mij;

/* ------------------------------------------------------------------ errors */

static thread_local char g_err[256] = "";

static int set_err(int code, const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_err, sizeof(g_err), fmt, ap);
	va_end(ap);
	return code;
}

#define HIP_TRY(expr)                                                                         \
	do {                                                                                       \
		hipError_t e_ = (expr);                                                                 \
		if (e_ != hipSuccess)                                                                   \
			return set_err(MIJ_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));            \
	} while (0)

extern "C" const char *mij_last_error(void) { return g_err; }
extern "C" int mij_abi_version(void) { return MIJ_ABI_VERSION; }

extern "C" int mij_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

/* ------------------------------------------------------------------ decode kernel families */

/* kernel families of a launch plan, in launch order.  MK_RS_FAST + RS_*: pass 2 compiled per resampler (k_resample_fast) */
enum { MK_PLANES = 0, MK_RESAMPLE, MK_RS_FAST, MK_420 = MK_RS_FAST + RS_KINDS, MK_422, MK_444, MK_GREY, MK_440, MK_420W, MK_440W /* k_fused420w / k_fused440w: 512 threads, wide pictures */, MK_420X /* 1024 threads: one workgroup per CU */, MK_420S, MK_420T /* 128 / 64 threads: narrow pictures */, MK_422W, MK_422X, MK_422S, MK_422T /* k_fused422 with 512 / 1024 / 128 / 64 threads */, MK_1X1C /* k_fused1x1c: RGB-tagged / CMYK / YCCK at 1x1 */, MK_420C, MK_440C /* column segments: a row of MCUs beyond a CU's LDS */, MK_SCALED /* + SC_*: reduced-size decode, k_scaled per layout */, MK_444R = MK_SCALED + SC_LAYOUTS, MK_GREYR, MK_1X1CR /* windowed forms of k_fused444 / k_fused_grey / k_fused1x1c: slots with a region (mij_batch_set_roi) */, MK_SCALEDR /* + SC_*: k_scaled on a window */, MK_PLANES_OUT = MK_SCALEDR + SC_LAYOUTS /* k_planes_out: slots with a plane request (mij_batch_set_out_planes) */, MK_LJ_IDCT /* libjpeg arithmetic (mij_batch_set_arith): k_lj_idct, pass 1 */, MK_LJ_COLOR /* + LJ_*: k_lj_color per chroma subsampling, pass 2 */, MK_KINDS = MK_LJ_COLOR + 4 };
/* the chroma subsamplings of k_lj_color; LJ_11 also takes one-component files and luma-only outputs */
enum { LJ_11 = 0, LJ_21, LJ_12, LJ_22 };

/* A family's kernels per variant = 4 * (n_out == 4) + 2 * wide IDCT + compact planes (k_resample_fast: 4 * (n_out == 4) + 2 * YCbCr
 * colour; k_scaled: 2 * (log2 of the scale - 1) + compact planes).  Every decode kernel takes (const DevImage *, const Work *, const uint8_t *in, uint8_t *out); io says which arenas in and
 * out are.  roi: a windowed form, which takes the batch's DevRoi table as a fifth argument; planes: k_planes_out, which takes the table of plane
 * requests there and writes the callers' memory, not the output arena. */
enum { MK_VARIANTS = 8 };
enum Arena { COEF_OUT, COEF_PLANES, PLANES_OUT };
struct Family {
	unsigned threads; /* workgroup size */
	Arena io;
	bool band; /* a band kernel: dynamic LDS up to the whole CU's */
	const void *k[MK_VARIANTS];
	bool roi, planes;
};
#define MIJ_K(...) reinterpret_cast<const void *>(&__VA_ARGS__)
#define MIJ_NWB(K)                                                                                                                  \
	{ MIJ_K(K<3, false, false>), MIJ_K(K<3, false, true>), MIJ_K(K<3, true, false>), MIJ_K(K<3, true, true>),                      \
	  MIJ_K(K<4, false, false>), MIJ_K(K<4, false, true>), MIJ_K(K<4, true, false>), MIJ_K(K<4, true, true>) }
#define MIJ_WB(K) { MIJ_K(K<false, false>), MIJ_K(K<false, true>), MIJ_K(K<true, false>), MIJ_K(K<true, true>) }
/* k_planes_out: 4 * (the slot's request has a paired form) + 2 * wide IDCT + compact planes */
#define MIJ_WBP(K)                                                                                                                  \
	{ MIJ_K(K<false, false, false>), MIJ_K(K<false, true, false>), MIJ_K(K<true, false, false>), MIJ_K(K<true, true, false>),       \
	  MIJ_K(K<false, false, true>), MIJ_K(K<false, true, true>), MIJ_K(K<true, false, true>), MIJ_K(K<true, true, true>) }
/* the windowed forms: the same kernels with the DevRoi table as fifth parameter */
#define MIJ_R const DevRoi *
#define MIJ_NWBR(K)                                                                                                                 \
	{ MIJ_K(K<3, false, false, MIJ_R>), MIJ_K(K<3, false, true, MIJ_R>), MIJ_K(K<3, true, false, MIJ_R>), MIJ_K(K<3, true, true, MIJ_R>),      \
	  MIJ_K(K<4, false, false, MIJ_R>), MIJ_K(K<4, false, true, MIJ_R>), MIJ_K(K<4, true, false, MIJ_R>), MIJ_K(K<4, true, true, MIJ_R>) }
#define MIJ_WBR(K) { MIJ_K(K<false, false, MIJ_R>), MIJ_K(K<false, true, MIJ_R>), MIJ_K(K<true, false, MIJ_R>), MIJ_K(K<true, true, MIJ_R>) }
#define MIJ_SC(Y) { MIJ_K(k_scaled<Y, 2, false>), MIJ_K(k_scaled<Y, 2, true>), MIJ_K(k_scaled<Y, 4, false>), MIJ_K(k_scaled<Y, 4, true>), MIJ_K(k_scaled<Y, 8, false>), MIJ_K(k_scaled<Y, 8, true>) }
#define MIJ_SCR(Y) { MIJ_K(k_scaled<Y, 2, false, MIJ_R>), MIJ_K(k_scaled<Y, 2, true, MIJ_R>), MIJ_K(k_scaled<Y, 4, false, MIJ_R>), MIJ_K(k_scaled<Y, 4, true, MIJ_R>), MIJ_K(k_scaled<Y, 8, false, MIJ_R>), MIJ_K(k_scaled<Y, 8, true, MIJ_R>) }
#define MIJ_RSF(R)                                                                                                                  \
	{ MIJ_K(k_resample_fast<R, false, 3>), nullptr, MIJ_K(k_resample_fast<R, true, 3>), nullptr,                                   \
	  MIJ_K(k_resample_fast<R, false, 4>), nullptr, MIJ_K(k_resample_fast<R, true, 4>), nullptr }
static const Family families[MK_KINDS] = {
	/* MK_PLANES */ {256, COEF_PLANES, false, MIJ_WB(k_idct_planes)},
	/* MK_RESAMPLE */ {256, PLANES_OUT, false, {MIJ_K(k_resample_color)}},
	{256, PLANES_OUT, false, MIJ_RSF(RS_ROW1)},
	{256, PLANES_OUT, false, MIJ_RSF(RS_V2)},
	{256, PLANES_OUT, false, MIJ_RSF(RS_H2)},
	{256, PLANES_OUT, false, MIJ_RSF(RS_HV2)},
	{256, PLANES_OUT, false, MIJ_RSF(RS_GEN2)},
	{256, PLANES_OUT, false, MIJ_RSF(RS_GEN4)},
	/* MK_420 */ {MIJ_F420_NT, COEF_OUT, true, MIJ_NWB(k_fused420)},
	/* MK_422 */ {MIJ_F420_NT, COEF_OUT, true, MIJ_NWB(k_fused422)},
	/* MK_444 */ {256, COEF_OUT, false, MIJ_NWB(k_fused444)},
	/* MK_GREY */ {256, COEF_OUT, false, MIJ_WB(k_fused_grey)},
	/* MK_440 */ {MIJ_F420_NT, COEF_OUT, true, MIJ_NWB(k_fused440)},
	/* MK_420W */ {MIJ_F420W_NT, COEF_OUT, true, MIJ_NWB(k_fused420w)},
	/* MK_440W */ {MIJ_F420W_NT, COEF_OUT, true, MIJ_NWB(k_fused440w)},
	/* MK_420X */ {MIJ_F420X_NT, COEF_OUT, true, MIJ_NWB(k_fused420x)},
	/* MK_420S */ {MIJ_F420S_NT, COEF_OUT, true, MIJ_NWB(k_fused420s)},
	/* MK_420T */ {MIJ_F420T_NT, COEF_OUT, true, MIJ_NWB(k_fused420t)},
	/* MK_422W */ {MIJ_F420W_NT, COEF_OUT, true, MIJ_NWB(k_fused422w)},
	/* MK_422X */ {MIJ_F420X_NT, COEF_OUT, true, MIJ_NWB(k_fused422x)},
	/* MK_422S */ {MIJ_F420S_NT, COEF_OUT, true, MIJ_NWB(k_fused422s)},
	/* MK_422T */ {MIJ_F420T_NT, COEF_OUT, true, MIJ_NWB(k_fused422t)},
	/* MK_1X1C */ {256, COEF_OUT, false, MIJ_NWB(k_fused1x1c)},
	/* MK_420C */ {MIJ_F420C_NT, COEF_OUT, true, MIJ_NWB(k_fused420c)},
	/* MK_440C */ {MIJ_F420C_NT, COEF_OUT, true, MIJ_NWB(k_fused440c)},
	/* MK_SCALED + SC_Y, SC_444, SC_420, SC_422 */
	{256, COEF_OUT, false, MIJ_SC(SC_Y)},
	{256, COEF_OUT, false, MIJ_SC(SC_444)},
	{256, COEF_OUT, false, MIJ_SC(SC_420)},
	{256, COEF_OUT, false, MIJ_SC(SC_422)},
	/* MK_444R */ {256, COEF_OUT, false, MIJ_NWBR(k_fused444), true},
	/* MK_GREYR */ {256, COEF_OUT, false, MIJ_WBR(k_fused_grey), true},
	/* MK_1X1CR */ {256, COEF_OUT, false, MIJ_NWBR(k_fused1x1c), true},
	/* MK_SCALEDR + SC_Y, SC_444, SC_420, SC_422 */
	{256, COEF_OUT, false, MIJ_SCR(SC_Y), true},
	{256, COEF_OUT, false, MIJ_SCR(SC_444), true},
	{256, COEF_OUT, false, MIJ_SCR(SC_420), true},
	{256, COEF_OUT, false, MIJ_SCR(SC_422), true},
	/* MK_PLANES_OUT */ {256, COEF_OUT, false, MIJ_WBP(k_planes_out), false, true},
	/* MK_LJ_IDCT: variant = compact planes */ {256, COEF_PLANES, false, {MIJ_K(k_lj_idct<false>), MIJ_K(k_lj_idct<true>)}},
	/* MK_LJ_COLOR + LJ_11, LJ_21, LJ_12, LJ_22: variant = n_out - 1 */
	{256, PLANES_OUT, false, {MIJ_K(k_lj_color<1, 1, 1>), MIJ_K(k_lj_color<1, 1, 2>), MIJ_K(k_lj_color<1, 1, 3>), MIJ_K(k_lj_color<1, 1, 4>)}},
	{256, PLANES_OUT, false, {nullptr, nullptr, MIJ_K(k_lj_color<2, 1, 3>), MIJ_K(k_lj_color<2, 1, 4>)}},
	{256, PLANES_OUT, false, {nullptr, nullptr, MIJ_K(k_lj_color<1, 2, 3>), MIJ_K(k_lj_color<1, 2, 4>)}},
	{256, PLANES_OUT, false, {nullptr, nullptr, MIJ_K(k_lj_color<2, 2, 3>), MIJ_K(k_lj_color<2, 2, 4>)}},
};
/* MK_420's pipelined twins (k_fused420p), by variant: compact planes without the wide IDCT only.  Not a family: a launch of MK_420 takes the twin of
 * its variant where band_prefetch says so, and everything that names a picture's kernel (kind, variant, segments) stays what it was. */
static const void *const k420_prefetch[MK_VARIANTS] = {nullptr, MIJ_K(k_fused420p<3>), nullptr, nullptr, nullptr, MIJ_K(k_fused420p<4>), nullptr, nullptr};
/* The twin needs more registers (MIJ_F420P_WAVES waves per SIMD), so it runs only where the launch's LDS allows no more workgroups per CU than that anyway */
static bool band_prefetch(int kind, int var, size_t lds, size_t cap)
{
	if (!MIJ_F420_PF || kind != MK_420 || !k420_prefetch[var] || !lds)
		return false;
	return (cap / lds) * (families[MK_420].threads / 64) <= 4 * MIJ_F420P_WAVES;
}
/* ... and the twins whose phase B marches down its lanes' own strips (k_fused420m), taken in their place where band_march says so */
static const void *const k420_march[MK_VARIANTS] = {nullptr, MIJ_K(k_fused420m<3>), nullptr, nullptr, nullptr, MIJ_K(k_fused420m<4>), nullptr, nullptr};
#undef MIJ_SCR
#undef MIJ_WBR
#undef MIJ_NWBR
#undef MIJ_R
#undef MIJ_SC
#undef MIJ_RSF
#undef MIJ_WBP
#undef MIJ_WB
#undef MIJ_NWB
#undef MIJ_K

/* ------------------------------------------------------------------ context */

struct mij_ctx {
	int device;
	hipDeviceProp_t prop;
	int max_dyn_lds;
	/* pinned bounce buffer of the one-slot fetches (d2h_bounced) */
	std::mutex bounce_lock;
	uint8_t *bounce = nullptr;
	hipEvent_t bounce_ev[2] = {nullptr, nullptr};
};
static const size_t MIJ_BOUNCE_BYTES = (size_t)8 << 20;

/* Device -> caller-owned host memory for the one-slot fetches (mij_batch_fetch, mij_enc_fetch, mij_batch_fetch_coef).  The caller's
 * buffer is ordinary pageable memory, often never touched before; handing it to hipMemcpyAsync makes the runtime pin, DMA into and
 * unpin pages this library does not own (or stage through a path shared by every stream of the process).  The
 * copy therefore lands in a pinned buffer of the context, 8 MiB at a time (two halves: the next chunk's DMA runs while the calling thread
 * copies this one out): the DMA engine only ever writes memory the library allocated with hipHostMalloc.  (Round 3: the one input of the
 * twice-seen encoder-leg mismatch that was not a pure function of its arguments was a DMA into a fresh numpy buffer, DESIGN.md
 * section 8.)  Throughput paths do not come here: they copy whole arenas into pinned memory the caller got from mij_host_alloc. */
static int d2h_bounced(mij_ctx *ctx, hipStream_t st, void *dst, const void *src_dev, size_t bytes);

extern "C" int mij_ctx_create(int device, mij_ctx **out)
{
	if (!out)
		return set_err(MIJ_E_ARG, "mij_ctx_create: out is NULL");
	*out = nullptr;
	int n = 0;
	hipError_t e = hipGetDeviceCount(&n);
	if (e != hipSuccess || n <= 0)
		return set_err(MIJ_E_NODEVICE, "no gpu device (%s)", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
	if (device < 0) {
		if (hipGetDevice(&device) != hipSuccess)
			device = 0;
	}
	if (device >= n)
		return set_err(MIJ_E_ARG, "device %d out of range (%d devices)", device, n);
	mij_ctx *c = new (std::nothrow) mij_ctx();
	if (!c)
		return set_err(MIJ_E_NOMEM, "out of host memory");
	c->device = device;
	if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&c->prop, device) != hipSuccess) {
		delete c;
		return set_err(MIJ_E_NODEVICE, "cannot open device %d", device);
	}
	if (strncmp(c->prop.gcnArchName, "gfx950", 6) != 0) {
		/* the kernels are built for gfx950 only; any other device cannot load the code object */
		set_err(MIJ_E_NODEVICE, "device %d is %s, this library is built for gfx950 only", device, c->prop.gcnArchName);
		delete c;
		return MIJ_E_NODEVICE;
	}
	c->max_dyn_lds = 160 * 1024;
	/* allow the fused band kernels to use the whole 160 KiB of LDS for wide images */
	for (const Family &f : families)
		if (f.band)
			for (const void *k : f.k)
				(void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, c->max_dyn_lds);
	for (const void *k : k420_prefetch)
		if (k)
			(void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, c->max_dyn_lds);
	for (const void *k : k420_march)
		if (k)
			(void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, c->max_dyn_lds);
	(void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_encode420), hipFuncAttributeMaxDynamicSharedMemorySize, MIJ_ENC_LDS);
	(void)hipGetLastError();
	*out = c;
	return MIJ_OK;
}

/* HIP gives a process four hardware queues by default and maps every further stream onto one of them; two batches that share
 * a queue run their kernels one after the other.  A ring of four batches plus one idle per-thread batch of stbi_load already loses
 * 30 % of its throughput that way (profiles/r02v_hw_queues.txt).  Unless the user chose a value, ask for eight -- this has to
 * happen before the HIP runtime initialises, hence a constructor of this library (a process that touched HIP earlier keeps its setting). */
__attribute__((constructor)) static void mij_hip_defaults() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

extern "C" void mij_ctx_destroy(mij_ctx *ctx)
{
	if (!ctx)
		return;
	if (ctx->bounce) {
		(void)hipSetDevice(ctx->device);
		(void)hipHostFree(ctx->bounce);
		for (int i = 0; i < 2; ++i)
			if (ctx->bounce_ev[i])
				(void)hipEventDestroy(ctx->bounce_ev[i]);
	}
	delete ctx;
}

static int d2h_bounced(mij_ctx *ctx, hipStream_t st, void *dst, const void *src_dev, size_t bytes)
{
	std::lock_guard<std::mutex> guard(ctx->bounce_lock);
	if (!ctx->bounce) {
		HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&ctx->bounce), 2 * MIJ_BOUNCE_BYTES, hipHostMallocDefault));
		HIP_TRY(hipEventCreateWithFlags(&ctx->bounce_ev[0], hipEventDisableTiming));
		HIP_TRY(hipEventCreateWithFlags(&ctx->bounce_ev[1], hipEventDisableTiming));
	}
	if (!bytes) {
		HIP_TRY(hipStreamSynchronize(st));
		return MIJ_OK;
	}
	/* two halves: the DMA of chunk k+1 runs while the calling thread copies chunk k out (a 4096 x 4096 picture is seven chunks) */
	const size_t nchunk = (bytes + MIJ_BOUNCE_BYTES - 1) / MIJ_BOUNCE_BYTES;
	for (size_t k = 0; k <= nchunk; ++k) {
		if (k < nchunk) {
			const size_t off = k * MIJ_BOUNCE_BYTES, n = bytes - off < MIJ_BOUNCE_BYTES ? bytes - off : MIJ_BOUNCE_BYTES;
			HIP_TRY(hipMemcpyAsync(ctx->bounce + (k & 1) * MIJ_BOUNCE_BYTES, static_cast<const uint8_t *>(src_dev) + off, n, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipEventRecord(ctx->bounce_ev[k & 1], st));
		}
		if (k > 0) {
			const size_t off = (k - 1) * MIJ_BOUNCE_BYTES, n = bytes - off < MIJ_BOUNCE_BYTES ? bytes - off : MIJ_BOUNCE_BYTES;
			HIP_TRY(hipEventSynchronize(ctx->bounce_ev[(k - 1) & 1]));
			memcpy(static_cast<uint8_t *>(dst) + off, ctx->bounce + ((k - 1) & 1) * MIJ_BOUNCE_BYTES, n);
		}
	}
	return MIJ_OK;
}
extern "C" int mij_ctx_device(const mij_ctx *ctx) { return ctx ? ctx->device : -1; }

extern "C" int mij_ctx_info(const mij_ctx *ctx, char *arch, size_t arch_len, int *cu_count, size_t *total_mem)
{
	if (!ctx)
		return set_err(MIJ_E_ARG, "ctx is NULL");
	if (arch && arch_len) {
		strncpy(arch, ctx->prop.gcnArchName, arch_len - 1);
		arch[arch_len - 1] = 0;
	}
	if (cu_count)
		*cu_count = ctx->prop.multiProcessorCount;
	if (total_mem)
		*total_mem = ctx->prop.totalGlobalMem;
	return MIJ_OK;
}

/* ------------------------------------------------------------------ batch */

/* the kernel family the last upload chose for a slot (mij_batch_slot_path) */
enum SlotPath { PATH_NONE = 0, PATH_420, PATH_TWO_PASS, PATH_444, PATH_422, PATH_GREY, PATH_440, PATH_1X1C, PATH_SCALED, PATH_PLANES_OUT, PATH_LIBJPEG };

/* what classify chose for a slot: the path, the family (MK_*) and variant whose work list takes its items (two-pass: pass 2's),
 * column segments per band, and the LDS of a whole row of MCUs (the band kernels) */
struct Choice {
	int path = PATH_NONE, kind = -1, var = 0, nseg = 1;
	size_t lds = 0;
};

struct Slot {
	mij_image_desc desc;
	DevImage dev;
	size_t stage_off;  /* byte offset in the staging arena (clones: the source's) */
	size_t coef_base;  /* byte offset of this image's region in the coefficient arena */
	size_t coef_bytes; /* bytes of that region (mij_image_coef_bytes: room for either format) */
	int clone_of;      /* -1: own staging */
	int dev_coef;      /* 1: the GPU entropy stage wrote the coefficient planes in HBM; nothing to upload */
	int es_index;      /* index into the entropy arena's scan list, or -1 */
	int coef_bytes_fmt; /* 1: compact planes in HBM (low bytes + escapes + DC array), 0: int16 tile layout */
	Choice choice;     /* of the last upload; path 0 none, 1 fused 4:2:0, 2 two-pass, 3 fused 4:4:4, 4 fused 4:2:2, 5 fused grey, 6 fused 4:4:0, 7 fused 1x1 colour, 8 reduced-size */
	int f32;           /* float output: index of the slot's request (mij_batch::f32_req), -1 none */
	int ten;           /* tensor output: index of the slot's request (mij_batch::ten_req), -1 none */
	int pln;           /* plane output: index of the slot's request (mij_batch::pln_req), -1 none */
	int scale;         /* reduced-size decode (mij_batch_set_scale): 1, 2, 4 or 8; the stored picture is out_w(s) x out_h(s) */
	int arith;         /* MIJ_ARITH_STB, or MIJ_ARITH_LIBJPEG (mij_batch_set_arith): the slot takes k_lj_idct and k_lj_color */
	/* region of interest: what was asked for (mij_batch_set_roi: roi_on and roi[] = x0, y0, w, h in stored pixels; mij_batch_set_roi_auto), and
	 * what the last upload made of it -- the region in force (reg, reg_px: none for two-pass slots and for windows that need every MCU), the
	 * decoded rectangle (rect) and the rectangle of lane units the windowed kernels count through (win) */
	bool roi_on, roi_auto, reg;
	int roi[4], reg_px[4], rect[4];
	DevRoi win;
	int work_items; /* of the last upload, on the slot's own family list (mij_batch_slot_work_items) */
	/* the row-extent table (mij.h): a byte per block row, component after component; all 3 until a producer that saw every block of the
	 * slot's rows hands its own in (mij_batch_set_row_classes), and 3 again whenever the staging is handed out.  Clones: their source's, at upload */
	std::vector<uint8_t> rowcls;
};
static inline size_t row_class_count(const mij_image_desc &d)
{
	size_t n = 0;
	for (int c = 0; c < d.ncomp; ++c)
		n += (size_t)d.comp[c].bh;
	return n;
}
static inline bool wants_region(const Slot &s) { return s.roi_on || s.roi_auto; }

/* the stored picture of a slot: what every consumer of its pixels sees */
static inline int out_w(const Slot &s) { return mij_scaled_dim(s.desc.width, s.scale); }
static inline int out_h(const Slot &s) { return mij_scaled_dim(s.desc.height, s.scale); }
static inline size_t out_px_bytes(const Slot &s) { return (size_t)s.desc.n_out * (size_t)out_w(s) * (size_t)out_h(s); }

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* one free per device / pinned pointer, which is left null */
template <typename T> static void free_dev(T *&p) { if (p) (void)hipFree(p); p = nullptr; }
template <typename T> static void free_host(T *&p) { if (p) (void)hipHostFree(p); p = nullptr; }

/* A list or an arena a batch or an encoder owns: `cap` elements in pinned memory, in device memory or (a list the host fills and a kernel
 * reads) in both.  alloc is for what has its size when it is made: the arenas, whose size the caller chose, and the per-slot tables.  The
 * lists are reallocated through Grow and nowhere else. */
enum { BUF_PINNED = 1, BUF_ON_DEVICE = 2 };
template <typename T, int SIDES = BUF_PINNED | BUF_ON_DEVICE>
struct Buf {
	T *h = nullptr, *d = nullptr;
	size_t cap = 0;
	Buf() = default;
	Buf &operator=(Buf &&o) /* o, a temporary, releases what this held */
	{
		std::swap(h, o.h), std::swap(d, o.d), std::swap(cap, o.cap);
		return *this;
	}
	~Buf() { release(); }
	void release()
	{
		free_host(h);
		free_dev(d);
		cap = 0;
	}
	hipError_t alloc(size_t n) /* exactly n elements, the pinned side first; an empty arena still has an address; cap stays 0 on failure */
	{
		release();
		hipError_t r = hipSuccess;
		if (SIDES & BUF_PINNED)
			r = hipHostMalloc(reinterpret_cast<void **>(&h), sizeof(T) * (n ? n : 16), hipHostMallocDefault);
		if (r == hipSuccess && (SIDES & BUF_ON_DEVICE))
			r = hipMalloc(reinterpret_cast<void **>(&d), sizeof(T) * (n ? n : 16));
		if (r == hipSuccess)
			cap = n;
		return r;
	}
};

/* Grows the lists of one upload step.  Copies and launches queued earlier may still read a list, so the first one that has to be
 * reallocated waits for the stream: one wait however many grow, none when none does.  A list grows to need + need / 2 + 64 elements;
 * exact() is for the scratch planes, which take what the upload needs and no more.  rc is the first failure, hip what the allocation
 * behind it answered. */
struct Grow {
	hipStream_t stream;
	bool waited = false;
	int rc = MIJ_OK;
	hipError_t hip = hipSuccess;
	explicit Grow(hipStream_t st) : stream(st) {}
	template <typename T, int SIDES>
	bool operator()(Buf<T, SIDES> &b, size_t need) /* true: b was reallocated */
	{
		return to(b, need, need + need / 2 + 64);
	}
	template <typename T, int SIDES>
	bool exact(Buf<T, SIDES> &b, size_t need)
	{
		return to(b, need, need);
	}

private:
	template <typename T, int SIDES>
	bool to(Buf<T, SIDES> &b, size_t need, size_t ncap)
	{
		static_assert(SIDES & BUF_ON_DEVICE, "only what a kernel reads grows");
		if (rc != MIJ_OK || need <= b.cap)
			return false;
		if (!waited) {
			const hipError_t r = hipStreamSynchronize(stream);
			if (r != hipSuccess) {
				rc = set_err(MIJ_E_HIP, "hipStreamSynchronize before growing a list failed: %s", hipGetErrorString(r));
				return false;
			}
			waited = true;
		}
		hip = b.alloc(ncap);
		if (hip != hipSuccess)
			rc = set_err(MIJ_E_HIP, "growing a list to %zu elements failed: %s", ncap, hipGetErrorString(hip));
		return rc == MIJ_OK;
	}
};

struct Work4 { /* WorkBand and WorkIdct are both four u32 */
	uint32_t a, b, c, d;
};

/* an output pass's plan -- descriptors, tables and work list -- in one pinned buffer and its device copy */
struct PlanBuf {
	Buf<uint8_t> buf;
	size_t items = 0, lut_at = 0, work_at = 0; /* work items of the last upload; byte offsets of the tables and the work list */
};

/* GPU entropy stage (mij_batch_entropy_*; see mij_entropy_kernels.h for the algorithm).  The arena holds everything the kernels touch
 * besides the coefficient planes: the unstuffed streams, per-scan descriptors and Huffman tables, three state words and a counter per
 * subsequence, a DC difference and an L1 accumulator per block, and five verdict words per scan.  Made by mij_batch_entropy_reserve. */
static const int ES_MAX_ROUNDS = 96;
enum EsVerdict { EV_ANOMALY = 0, EV_CHANGED, EV_TOTAL, EV_L1MAX, EV_PFINAL, EV_ROWS }; /* the rows of the verdict table, scan_cap words each */
struct EsArena {
	Buf<uint8_t> stream; /* h: the pinned region the host stage writes the unstuffed streams into; cap bytes */
	Buf<DevScan> scans;  /* scan_cap */
	Buf<DevHuff> huff;   /* eight per table set */
	Buf<EsWork> work;
	Buf<WorkIdct> pack; /* k_es_pack: (slot, component, first block) per 256 blocks of every compact-plane slot */
	Buf<uint64_t, BUF_ON_DEVICE> start, end[2]; /* end[0]: the cold pass's end states, end[1]: the current ones (first round on) */
	Buf<uint4, BUF_ON_DEVICE> uni;  /* k_es_tables: one EsUni per table set */
	Buf<uint4, BUF_ON_DEVICE> wtab; /* ... and one EsW (the record-form write pass's tables) */
	Buf<uint32_t> tabscan;          /* table set -> a scan that uses it */
	Buf<uint32_t, BUF_ON_DEVICE> qidx[2];   /* the queues of k_es_syncq, alternating by round: subsequence ... */
	Buf<uint64_t, BUF_ON_DEVICE> qstate[2]; /* ... and the start state it has to run from; a scan's entries start at its sub_off */
	Buf<uint32_t, BUF_ON_DEVICE> cnt, base;
	size_t sub_cap = 0;    /* subsequences: start, end, the queues, cnt and base */
	uint32_t sub_bits = 0; /* bits per subsequence of this arena's scans */
	int rounds0 = 0;       /* synchronisation rounds queued before the first look at the verdicts */
	Buf<uint64_t, BUF_ON_DEVICE> meta; /* per block: L1 of its AC coefficients | DC difference << 32 */
	/* compact planes, the write pass's intermediate form: the zigzag image, 64 bytes per block, or with use_records the record form
	 * (k_es_writer / k_es_pack2), rec_region64 eight-byte words per subsequence.  Only one of the two is allocated. */
	Buf<uint8_t, BUF_ON_DEVICE> zz;
	Buf<uint64_t, BUF_ON_DEVICE> rec;
	uint32_t rec_region64 = 0;
	size_t rec_words = 0;
	bool use_records = false;
	size_t blk_cap = 0;
	Buf<uint32_t, BUF_ON_DEVICE> verdict; /* [EV_ROWS][scan_cap] */
	Buf<uint32_t, BUF_PINNED> verdict_host;
	Buf<uint32_t, BUF_ON_DEVICE> rounds_changed; /* [ES_MAX_ROUNDS]: k_es_tails' scratch */
	Buf<uint32_t, BUF_ON_DEVICE> changed; /* [ES_MAX_ROUNDS][scan_cap]: subsequences moved per scan, one slice per synchronisation round -- cleared once
	                                       * per launch instead of once per round (a one-picture batch queues 24 rounds: 24 fewer commands per stbi_load call) */
	std::vector<int> scan_slot; /* scan index -> batch slot */
	size_t sub_used = 0, blk_used = 0, work_used = 0, pack_used = 0, scan_cap = 0, n_tabs = 0;
	int last_rounds = 0;
	bool in_flight = false;

	uint32_t *d_row(EsVerdict v) { return verdict.d + (size_t)v * scan_cap; }
	const uint32_t *h_row(EsVerdict v) const { return verdict_host.h + (size_t)v * scan_cap; }
	uint32_t *h_row(EsVerdict v) { return verdict_host.h + (size_t)v * scan_cap; }
	void reset() /* mij_batch_reset: no scans, nothing in flight */
	{
		scan_slot.clear();
		sub_used = blk_used = work_used = pack_used = n_tabs = 0;
		in_flight = false;
	}
};

struct mij_batch {
	mij_ctx *ctx = nullptr;
	hipStream_t stream = nullptr;
	hipEvent_t ev_begin = nullptr, ev_end = nullptr;
	hipEvent_t ev_pack0 = nullptr, ev_pack1 = nullptr; /* around k_pack_c8 in the last upload (mij_batch_pack_ms); created on first use */
	bool pack_timed = false;
	int max_images = 0;
	/* the arenas, in bytes: pinned staging, coefficient planes, pixels, the two-pass path's scratch sample planes (as large as the largest
	 * upload needed), and the upload scratch: int16 planes on their way into compact planes (k_pack_c8), as large as the staging arena,
	 * made by the first upload that packs */
	Buf<uint8_t, BUF_PINNED> stage;
	Buf<uint8_t, BUF_ON_DEVICE> coef, out, planes, up16;
	size_t stage_used = 0, coef_used = 0, out_used = 0;
	/* per slot, max_images entries: the descriptors; the largest per-block L1 the pack kernel saw (MIJ_FLAG_L1_ON_DEVICE) and the windows
	 * of the windowed kernels, both made by the first upload that needs them */
	Buf<DevImage> imgs;
	/* the slots' row-extent tables as the band kernels read them (DevImage.rc_off): laid out by every upload in pinned memory, as much as it
	 * needs, and copied to the head of the coefficient arena -- rc_room bytes in front of the first slot's planes, room for a byte per
	 * block row of whatever fits the arena (a block row is at least one block, 130 bytes of its tile; the kernels' form is a byte per MCU
	 * row) and eight bytes of slack per slot */
	Buf<uint8_t, BUF_PINNED> rowcls;
	size_t rc_room = 0;
	Buf<uint32_t> l1max;
	Buf<DevRoi> roi;
	Buf<Work4> work; /* the work lists: the pack list, then one range per launch */
	std::vector<Slot> slots;
	/* launch plan built by upload: one per non-empty (family, variant) work list */
	struct Launch {
		int kind, var;
		size_t first, count, lds;
		bool marched; /* a pipelined launch of MK_420 that takes k_fused420m (band_march) */
	};
	std::vector<Launch> launches;
	bool uploaded = false, launched = false;
	int force_generic = 0; /* 0: fused kernels where they apply; 1: two-pass path for every image; 2: and its run-time-general pass 2 */
	int coef_fmt = 1;  /* format new coefficient planes get in HBM: 1 compact (default), 0 int16 (MIJ_COEF_FORMAT=int16, mij_batch_set_coef_format) */
	int band_rows = 0; /* MCU rows per fused workgroup; 0 = automatic */
	std::unique_ptr<EsArena> es; /* GPU entropy stage, made by mij_batch_entropy_reserve */
	/* float output (mij_batch_set_out_f32): the arena, one request per slot that asked (its place in the arena and its tables), and what
	 * upload made of them for k_out_f32 -- descriptors, tables and (slot, chunk) work list */
	Buf<uint8_t, BUF_ON_DEVICE> f32;
	size_t f32_used = 0;
	struct F32Req {
		int slot;
		size_t off;
		float lut[MIJ_F32_LUT_FLOATS];
	};
	std::vector<F32Req> f32_req;
	PlanBuf f32plan;
	/* tensor output (mij_batch_set_out_tensor): one validated request per slot that asked, and what upload made of them for
	 * k_out_tensor -- descriptors, tables and (request, rows, columns) work list */
	struct RszCoef {
		std::vector<int32_t> v; /* lo, n pairs [out][2], then taps [out][ks] */
		int ks;
		bool big, fits; /* some |k| >= 2^23; 255 * sum |k| + 2^21 < 2^31 for every output */
	};
	struct TenReq {
		int slot;
		mij_out_tensor t; /* in the stored picture's frame: an oriented request's mirrors are folded into the window and flips */
		bool tr;          /* orientations 5..8: transposed (k_out_tensor_t / k_out_resize_t; DevTensor's transposed meaning) */
		bool rsz; /* a resized request: r, and the coefficients of its axes (mirrored where the orientation mirrors that axis) */
		mij_out_resize r;
		const RszCoef *ch, *cv;
		uint32_t esize;
		bool lut;
		uint8_t table[MIJ_TEN_LUT_BYTES];
	};
	std::vector<TenReq> ten_req;
	PlanBuf tenplan;
	/* resized tensor output (mij_batch_set_out_tensor_resized): coefficients per (in, out, filter), kept until reset (std::map: the
	 * requests point at them), and k_out_resize's plan -- descriptors, tables, coefficients and work list -- in a buffer pair of its own */
	std::map<uint64_t, RszCoef> rsz_coef;
	/* plane output (mij_batch_set_out_planes): one validated request per slot that asked, as k_planes_out reads it (a component that is
	 * not wanted has dst 0), and the per-slot table the kernel takes, max_images entries, made by the first upload that needs it */
	struct PlnReq {
		int slot;
		DevPlanes dev;
	};
	std::vector<PlnReq> pln_req;
	Buf<DevPlanes> pln;
	PlanBuf rszplan;
	/* oriented tensor output with orientations 5..8 (mij_batch_set_out_tensor_oriented): k_out_tensor_t's and k_out_resize_t's plans */
	PlanBuf tentplan, rsztplan;
};

/* the slot, or null with MIJ_E_ARG and `what` as the error text */
static const Slot *batch_slot(const mij_batch *b, int slot, const char *what = "bad slot")
{
	if (!b || slot < 0 || slot >= (int)b->slots.size()) {
		set_err(MIJ_E_ARG, "%s", what);
		return nullptr;
	}
	return &b->slots[(size_t)slot];
}
static Slot *batch_slot(mij_batch *b, int slot, const char *what = "bad slot")
{
	return const_cast<Slot *>(batch_slot(static_cast<const mij_batch *>(b), slot, what));
}

static inline size_t comp_tiles(const mij_comp_desc &cp) { return ((size_t)(cp.bw * cp.bh) + 63) >> 6; }

/* room for either format: int16 tile layout needs 8192 B per 64-block tile, compact planes 4096 (low bytes) + 128 (DC)
 * + 4096 (escape bytes) = MIJ_TILE_COMPACT_BYTES */
extern "C" size_t mij_image_coef_bytes(const mij_image_desc *d)
{
	size_t total = 0;
	for (int c = 0; c < d->ncomp; ++c)
		total += comp_tiles(d->comp[c]) * MIJ_TILE_COMPACT_BYTES;
	return total;
}

extern "C" size_t mij_image_out_bytes(const mij_image_desc *d) { return align_up((size_t)d->n_out * d->width * d->height, 256); }

extern "C" int mij_batch_create(mij_ctx *ctx, int max_images, size_t stage_bytes, size_t coef_bytes, size_t out_bytes, mij_batch **out)
{
	if (!ctx || !out || max_images <= 0)
		return set_err(MIJ_E_ARG, "mij_batch_create: bad argument");
	*out = nullptr;
	HIP_TRY(hipSetDevice(ctx->device));
	mij_batch *b = new (std::nothrow) mij_batch();
	if (!b)
		return set_err(MIJ_E_NOMEM, "out of host memory");
	b->ctx = ctx;
	b->max_images = max_images;
	const char *fmt = getenv("MIJ_COEF_FORMAT");
	b->coef_fmt = (fmt && (!strcmp(fmt, "int16") || !strcmp(fmt, "0"))) ? 0 : 1;
	const char *env = getenv("MIJ_BAND_ROWS");
	if (env)
		b->band_rows = atoi(env);

	hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
	if (e == hipSuccess)
		e = hipEventCreate(&b->ev_begin);
	if (e == hipSuccess)
		e = hipEventCreate(&b->ev_end);
	if (e == hipSuccess && stage_bytes)
		e = b->stage.alloc(stage_bytes);
	if (e == hipSuccess && coef_bytes)
		e = b->coef.alloc(coef_bytes + (b->rc_room = align_up(coef_bytes / 130 + 8 * (size_t)max_images + 16, 4096)));
	b->coef_used = b->rc_room;
	if (e == hipSuccess && out_bytes)
		e = b->out.alloc(out_bytes);
	if (e == hipSuccess)
		e = b->imgs.alloc((size_t)max_images);
	if (e != hipSuccess) {
		int code = (e == hipErrorOutOfMemory) ? MIJ_E_NOMEM : MIJ_E_HIP;
		set_err(code, "mij_batch_create: %s", hipGetErrorString(e));
		mij_batch_destroy(b);
		return code;
	}
	b->slots.reserve((size_t)max_images);
	*out = b;
	return MIJ_OK;
}

extern "C" void mij_batch_destroy(mij_batch *b)
{
	if (!b)
		return;
	(void)hipSetDevice(b->ctx->device);
	if (b->stream)
		(void)hipStreamSynchronize(b->stream);
	const hipStream_t stream = b->stream;
	const hipEvent_t events[] = {b->ev_begin, b->ev_end, b->ev_pack0, b->ev_pack1};
	delete b; /* its buffers and its entropy arena release themselves, before the events and the stream go */
	for (hipEvent_t ev : events)
		if (ev)
			(void)hipEventDestroy(ev);
	if (stream)
		(void)hipStreamDestroy(stream);
}

extern "C" int mij_batch_reset(mij_batch *b)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	HIP_TRY(hipSetDevice(b->ctx->device));
	HIP_TRY(hipStreamSynchronize(b->stream));
	b->slots.clear();
	b->stage_used = b->out_used = 0;
	b->coef_used = b->rc_room;
	b->uploaded = b->launched = false;
	b->launches.clear();
	b->f32_req.clear();
	b->f32_used = 0;
	b->ten_req.clear();
	b->pln_req.clear();
	b->rsz_coef.clear();
	b->f32plan.items = b->tenplan.items = b->rszplan.items = b->tentplan.items = b->rsztplan.items = 0;
	if (b->es)
		b->es->reset();
	return MIJ_OK;
}

static int check_desc(const mij_image_desc *d)
{
	if (!d)
		return set_err(MIJ_E_ARG, "descriptor is NULL");
	if (d->width <= 0 || d->height <= 0 || d->width > 65535 || d->height > 65535)
		return set_err(MIJ_E_ARG, "bad image size %dx%d", d->width, d->height);
	if (!(d->ncomp == 1 || d->ncomp == 3 || d->ncomp == 4))
		return set_err(MIJ_E_ARG, "bad component count %d", d->ncomp);
	if (d->n_out < 1 || d->n_out > 4)
		return set_err(MIJ_E_ARG, "bad n_out %d", d->n_out);
	if (d->color < MIJ_COLOR_GREY || d->color > MIJ_COLOR_YCBCRA)
		return set_err(MIJ_E_ARG, "bad colour mode %d", d->color);
	if ((d->color == MIJ_COLOR_YCBCR || d->color == MIJ_COLOR_RGB) && d->ncomp != 3)
		return set_err(MIJ_E_ARG, "colour mode %d needs 3 components", d->color);
	if (d->color >= MIJ_COLOR_CMYK && d->ncomp != 4)
		return set_err(MIJ_E_ARG, "colour mode %d needs 4 components", d->color);
	if (d->h_max < 1 || d->h_max > 4 || d->v_max < 1 || d->v_max > 4 || d->mcu_x <= 0 || d->mcu_y <= 0)
		return set_err(MIJ_E_ARG, "bad MCU geometry");
	for (int c = 0; c < d->ncomp; ++c) {
		const mij_comp_desc &cp = d->comp[c];
		if (cp.h < 1 || cp.h > 4 || cp.v < 1 || cp.v > 4 || cp.tq < 0 || cp.tq > 3)
			return set_err(MIJ_E_ARG, "bad sampling/table for component %d", c);
		if (cp.h > d->h_max || cp.v > d->v_max)
			return set_err(MIJ_E_ARG, "component %d sampling exceeds h_max/v_max", c);
		if (cp.bw != d->mcu_x * cp.h || cp.bh != d->mcu_y * cp.v)
			return set_err(MIJ_E_ARG, "component %d block grid does not match the MCU grid", c);
		if (cp.x <= 0 || cp.y <= 0 || cp.x > cp.bw * 8 || cp.y > cp.bh * 8)
			return set_err(MIJ_E_ARG, "component %d effective size out of range", c);
	}
	/* the MCU grid covers the picture (codec/jpeg.c:1618-1622): the kernels address pixels from MCU coordinates */
	if ((int64_t)d->width > (int64_t)d->mcu_x * 8 * d->h_max || (int64_t)d->height > (int64_t)d->mcu_y * 8 * d->v_max)
		return set_err(MIJ_E_ARG, "image larger than its MCU grid");
	return MIJ_OK;
}

/* where the component planes of a slot lie inside its region of the coefficient arena, for its format */
static void layout_coef(Slot &s)
{
	size_t off = s.coef_base;
	if (s.coef_bytes_fmt)
		s.dev.flags |= MIJ_DEV_COEF_BYTES;
	else
		s.dev.flags &= ~(int32_t)MIJ_DEV_COEF_BYTES;
	for (int c = 0; c < s.desc.ncomp; ++c) {
		const size_t nt = comp_tiles(s.desc.comp[c]);
		DevComp &dc = s.dev.comp[c];
		if (s.coef_bytes_fmt) { /* mij.h, mij_compact_offsets: low bytes + DC of every component first, the escape bytes behind them */
			size_t lo, dcv, hi;
			mij_compact_offsets(&s.desc, c, &lo, &dcv, &hi);
			dc.coef_off = s.coef_base + lo;
			dc.dc_off = s.coef_base + dcv;
			dc.hi_off = s.coef_base + hi;
		} else {
			dc.coef_off = off;
			dc.dc_off = dc.hi_off = 0;
			off += nt << 13;
		}
	}
}

/* quantisation tables, natural order -> in-block position order P = 8*col + rowslot[row] */
static void fill_dev_dequant(Slot &s)
{
	const mij_image_desc &d = s.desc;
	for (int c = 0; c < d.ncomp; ++c) {
		uint16_t q[64];
		for (int row = 0; row < 8; ++row)
			for (int col = 0; col < 8; ++col)
				q[8 * col + mij_rowslot[row]] = d.dequant[d.comp[c].tq][8 * row + col];
		for (int i = 0; i < 32; ++i)
			s.dev.dq[c][i] = (uint32_t)q[2 * i] | ((uint32_t)q[2 * i + 1] << 16);
	}
}

static void fill_dev_image(Slot &s, size_t out_off)
{
	const mij_image_desc &d = s.desc;
	DevImage &v = s.dev;
	memset(&v, 0, sizeof(v));
	v.width = d.width;
	v.height = d.height;
	v.n_out = d.n_out;
	v.color = d.color;
	v.ncomp = d.ncomp;
	v.flags = (int32_t)d.flags;
	v.mcu_x = d.mcu_x;
	v.mcu_y = d.mcu_y;
	v.out_off = out_off;
	size_t plane_off = 0;
	for (int c = 0; c < d.ncomp; ++c) {
		DevComp &dc = v.comp[c];
		const mij_comp_desc &cp = d.comp[c];
		dc.h = cp.h;
		dc.v = cp.v;
		dc.x = cp.x;
		dc.y = cp.y;
		dc.bw = cp.bw;
		dc.bh = cp.bh;
		dc.hs = d.h_max / cp.h;
		dc.vs = d.v_max / cp.v;
		dc.plane_off = plane_off; /* relative; rebased at launch */
		plane_off += align_up((size_t)cp.bw * 8 * cp.bh * 8, 256);
	}
	v.plane_bytes_total = plane_off;
	fill_dev_dequant(s);
}

#define MIJ_NO_STAGE ((size_t)-1)

/* lazy_stage: a slot of the GPU entropy stage -- its staging planes are only needed if the host walk has to
 * redo it, so they are neither required nor cleared here (mij_batch_fallback_prepare does that) */
static int add_common(mij_batch *b, const mij_image_desc *d, int clone_of, bool lazy_stage = false, bool clear = true)
{
	if ((int)b->slots.size() >= b->max_images)
		return set_err(MIJ_E_NOMEM, "batch is full (%d images)", b->max_images);
	const size_t cbytes = mij_image_coef_bytes(d), obytes = mij_image_out_bytes(d);
	if (b->coef_used + cbytes > b->coef.cap)
		return set_err(MIJ_E_NOMEM, "coefficient arena exhausted");
	if (b->out_used + obytes > b->out.cap)
		return set_err(MIJ_E_NOMEM, "output arena exhausted");
	Slot s;
	s.desc = *d;
	s.clone_of = clone_of;
	s.dev_coef = 0;
	s.es_index = -1;
	s.coef_bytes_fmt = clone_of >= 0 ? b->slots[(size_t)clone_of].coef_bytes_fmt : 0;
	s.coef_bytes = cbytes;
	s.choice = Choice();
	s.f32 = -1;
	s.ten = -1;
	s.pln = -1;
	s.scale = 1;
	s.arith = MIJ_ARITH_STB;
	s.roi_on = s.roi_auto = s.reg = false;
	s.work_items = 0;
	s.rowcls.assign(row_class_count(*d), (uint8_t)3);
	if (clone_of < 0) {
		if (b->stage_used + cbytes > b->stage.cap) {
			if (!lazy_stage)
				return set_err(MIJ_E_NOMEM, "staging arena exhausted");
			s.stage_off = MIJ_NO_STAGE;
		} else {
			s.stage_off = b->stage_used;
			if (!lazy_stage && clear)
				memset(b->stage.h + s.stage_off, 0, cbytes);
			b->stage_used += cbytes;
		}
	} else {
		s.stage_off = b->slots[(size_t)clone_of].stage_off;
	}
	s.coef_base = b->coef_used;
	fill_dev_image(s, b->out_used);
	layout_coef(s); /* host-staged slots: int16 until upload decides; clones: their source's format */
	b->coef_used += cbytes;
	b->out_used += obytes;
	b->slots.push_back(s);
	b->uploaded = b->launched = false;
	return (int)b->slots.size() - 1;
}

extern "C" int mij_batch_add(mij_batch *b, const mij_image_desc *d)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	int rc = check_desc(d);
	if (rc != MIJ_OK)
		return rc;
	return add_common(b, d, -1);
}

extern "C" int mij_batch_add_uncleared(mij_batch *b, const mij_image_desc *d)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	int rc = check_desc(d);
	if (rc != MIJ_OK)
		return rc;
	return add_common(b, d, -1, false, false);
}

extern "C" int mij_batch_add_clone(mij_batch *b, int src_slot)
{
	if (!batch_slot(b, src_slot, "bad source slot"))
		return MIJ_E_ARG;
	int root = b->slots[(size_t)src_slot].clone_of >= 0 ? b->slots[(size_t)src_slot].clone_of : src_slot;
	mij_image_desc d = b->slots[(size_t)root].desc;
	return add_common(b, &d, root);
}

extern "C" int16_t *mij_batch_coef(mij_batch *b, int slot, int comp)
{
	if (!batch_slot(b, slot))
		return nullptr;
	Slot &s = b->slots[(size_t)slot];
	if (comp < 0 || comp >= s.desc.ncomp || s.clone_of >= 0 || !b->stage.h || s.stage_off == MIJ_NO_STAGE) {
		set_err(MIJ_E_ARG, "bad component, or slot has no staging of its own");
		return nullptr;
	}
	std::fill(s.rowcls.begin(), s.rowcls.end(), (uint8_t)3); /* whoever asks for the staging is about to write it */
	size_t off = s.stage_off;
	for (int c = 0; c < comp; ++c)
		off += mij_plane_elems((uint32_t)(s.desc.comp[c].bw * s.desc.comp[c].bh)) * sizeof(int16_t);
	return reinterpret_cast<int16_t *>(b->stage.h + off);
}

extern "C" uint8_t *mij_batch_stage_region(mij_batch *b, int slot, size_t *bytes)
{
	if (!batch_slot(b, slot))
		return nullptr;
	Slot &s = b->slots[(size_t)slot];
	if (s.clone_of >= 0 || !b->stage.h || s.stage_off == MIJ_NO_STAGE) {
		set_err(MIJ_E_ARG, "slot has no staging of its own");
		return nullptr;
	}
	if (bytes)
		*bytes = s.coef_bytes;
	std::fill(s.rowcls.begin(), s.rowcls.end(), (uint8_t)3); /* whoever asks for the staging is about to write it */
	return b->stage.h + s.stage_off;
}

extern "C" int mij_batch_set_row_classes(mij_batch *b, int slot, const uint8_t *classes, size_t n)
{
	Slot *s = batch_slot(b, slot);
	if (!s)
		return MIJ_E_ARG;
	if (!classes || n != s->rowcls.size() || s->clone_of >= 0)
		return set_err(MIJ_E_ARG, "mij_batch_set_row_classes: slot %d has %zu block rows of its own staging", slot, s->clone_of >= 0 ? (size_t)0 : s->rowcls.size());
	for (size_t i = 0; i < n; ++i)
		s->rowcls[i] = classes[i] < 3 ? classes[i] : (uint8_t)3;
	b->uploaded = b->launched = false;
	return MIJ_OK;
}

extern "C" int mij_batch_fetch_row_classes_packed(mij_batch *b, int slot, uint8_t *dst, size_t cap)
{
	const Slot *s = batch_slot(b, slot);
	if (!s)
		return MIJ_E_ARG;
	if (!b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_fetch_row_classes_packed before mij_batch_upload");
	const size_t n = (size_t)s->desc.mcu_y;
	if (dst && cap >= n) {
		HIP_TRY(hipSetDevice(b->ctx->device));
		const int rc = d2h_bounced(b->ctx, b->stream, dst, b->coef.d + s->dev.rc_off, n);
		if (rc != MIJ_OK)
			return rc;
	}
	return (int)n;
}

extern "C" int mij_batch_slot_row_classes(const mij_batch *b, int slot, uint8_t *dst, size_t cap)
{
	const Slot *s = batch_slot(b, slot);
	if (!s)
		return MIJ_E_ARG;
	const Slot &src = s->clone_of >= 0 ? b->slots[(size_t)s->clone_of] : *s; /* what the next upload gives a clone */
	if (dst && cap >= src.rowcls.size())
		memcpy(dst, src.rowcls.data(), src.rowcls.size());
	return (int)src.rowcls.size();
}

extern "C" int mij_batch_coef_format(const mij_batch *b) { return b ? b->coef_fmt : MIJ_COEF_COMPACT; }
extern "C" uint32_t mij_batch_slot_flags(const mij_batch *b, int slot)
{
	if (!batch_slot(b, slot))
		return 0;
	return b->slots[(size_t)slot].desc.flags;
}

extern "C" int mij_batch_set_flags(mij_batch *b, int slot, uint32_t flags)
{
	if (!batch_slot(b, slot))
		return MIJ_E_ARG;
	b->slots[(size_t)slot].desc.flags = flags;
	b->slots[(size_t)slot].dev.flags = (int32_t)flags | (b->slots[(size_t)slot].coef_bytes_fmt ? MIJ_DEV_COEF_BYTES : 0);
	b->uploaded = b->launched = false;
	return MIJ_OK;
}

/* Which k_scaled layout (SC_*) decodes a picture at reduced size, or -1: one component; or three-component YCbCr (its luma alone when
 * fewer than three channels are asked for) whose luma has the picture's resolution and whose chroma is 4:4:4, 4:2:0 or 4:2:2 -- the
 * layouts where every transform length N * h_max / h, N * v_max / v stays within 8 and all components land on one grid. */
static int scaled_layout(const mij_image_desc &d)
{
	if ((uint64_t)d.width * d.height * d.n_out >= 0xfffffff0ull)
		return -1;
	if (d.ncomp == 1 && d.color == MIJ_COLOR_GREY)
		return SC_Y;
	if (d.ncomp != 3 || (d.color != MIJ_COLOR_YCBCR && d.color != MIJ_COLOR_GREY) || (d.color == MIJ_COLOR_GREY && d.n_out >= 3))
		return -1;
	if (d.comp[0].h != d.h_max || d.comp[0].v != d.v_max || d.comp[1].h != 1 || d.comp[1].v != 1 || d.comp[2].h != 1 || d.comp[2].v != 1)
		return -1;
	const int lay = (d.h_max == 1 && d.v_max == 1) ? SC_444 : (d.h_max == 2 && d.v_max == 2) ? SC_420 : (d.h_max == 2 && d.v_max == 1) ? SC_422 : -1;
	return (lay < 0 || d.n_out >= 3) ? lay : SC_Y;
}

extern "C" int mij_batch_set_scale(mij_batch *b, int slot, int denom)
{
	if (!batch_slot(b, slot, "mij_batch_set_scale: bad slot"))
		return MIJ_E_ARG;
	if (b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_set_scale after mij_batch_upload");
	Slot &s = b->slots[(size_t)slot];
	if (s.desc.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_STATE, "slot %d was rejected by the host stage", slot);
	if (denom != 1 && denom != 2 && denom != 4 && denom != 8)
		return set_err(MIJ_E_ARG, "mij_batch_set_scale: denominator %d is not 1, 2, 4 or 8", denom);
	if (denom > 1 && scaled_layout(s.desc) < 0)
		return set_err(MIJ_E_ARG, "mij_batch_set_scale: slot %d cannot be decoded at reduced size (grey, or YCbCr 4:4:4 / 4:2:0 / 4:2:2 only; "
										  "%d components, colour mode %d, luma %dx%d of %dx%d)", slot, s.desc.ncomp, s.desc.color, s.desc.comp[0].h, s.desc.comp[0].v, s.desc.h_max, s.desc.v_max);
	if (denom > 1 && s.arith == MIJ_ARITH_LIBJPEG)
		return set_err(MIJ_E_ARG, "mij_batch_set_scale: slot %d is decoded with libjpeg's arithmetic, which has no reduced-size form", slot);
	if (denom > 1 && s.f32 >= 0)
		return set_err(MIJ_E_ARG, "mij_batch_set_scale: slot %d has a float output request; float output of reduced pictures is not supported", slot);
	if (denom > 1 && s.pln >= 0)
		return set_err(MIJ_E_STATE, "mij_batch_set_scale: slot %d has a plane request; planes are not decoded at reduced size", slot);
	if (denom != s.scale && s.ten >= 0)
		return set_err(MIJ_E_STATE, "mij_batch_set_scale: slot %d already has a tensor request for its %dx%d picture; set the scale first", slot, out_w(s), out_h(s));
	s.scale = denom;
	return MIJ_OK;
}

/* Which k_lj_color form (LJ_*) decodes a picture with libjpeg's arithmetic, or -1: one component; or three-component YCbCr whose luma has
 * the picture's resolution and whose chroma planes share 4:4:4, 4:2:2, 4:4:0 or 4:2:0 subsampling (fewer than three channels: the luma alone) */
static int lj_layout(const mij_image_desc &d)
{
	if (d.n_out < 1 || d.n_out > 4)
		return -1;
	if (d.ncomp == 1 && d.color == MIJ_COLOR_GREY)
		return LJ_11;
	if (d.ncomp != 3 || (d.color != MIJ_COLOR_YCBCR && !(d.color == MIJ_COLOR_GREY && d.n_out < 3)))
		return -1;
	if (d.comp[0].h != d.h_max || d.comp[0].v != d.v_max || d.comp[1].h != d.comp[2].h || d.comp[1].v != d.comp[2].v)
		return -1;
	if (d.h_max % d.comp[1].h || d.v_max % d.comp[1].v)
		return -1;
	const int hs = d.h_max / d.comp[1].h, vs = d.v_max / d.comp[1].v;
	if (hs < 1 || hs > 2 || vs < 1 || vs > 2)
		return -1;
	return d.n_out < 3 ? LJ_11 : (hs == 2 ? (vs == 2 ? LJ_22 : LJ_21) : (vs == 2 ? LJ_12 : LJ_11));
}

extern "C" int mij_batch_set_arith(mij_batch *b, int slot, int arith)
{
	if (!batch_slot(b, slot, "mij_batch_set_arith: bad slot"))
		return MIJ_E_ARG;
	if (b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_set_arith after mij_batch_upload");
	Slot &s = b->slots[(size_t)slot];
	if (s.desc.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_STATE, "slot %d was rejected by the host stage", slot);
	if (arith != MIJ_ARITH_STB && arith != MIJ_ARITH_LIBJPEG)
		return set_err(MIJ_E_ARG, "mij_batch_set_arith: arithmetic %d is neither MIJ_ARITH_STB nor MIJ_ARITH_LIBJPEG", arith);
	if (arith == MIJ_ARITH_LIBJPEG) {
		if (lj_layout(s.desc) < 0)
			return set_err(MIJ_E_ARG, "mij_batch_set_arith: slot %d cannot be decoded with libjpeg's arithmetic (grey, or YCbCr 4:4:4 / 4:2:2 / 4:4:0 / 4:2:0 only; "
											  "%d components, colour mode %d, luma %dx%d of %dx%d)", slot, s.desc.ncomp, s.desc.color, s.desc.comp[0].h, s.desc.comp[0].v, s.desc.h_max, s.desc.v_max);
		if (s.scale > 1)
			return set_err(MIJ_E_ARG, "mij_batch_set_arith: slot %d is decoded at 1/%d size; libjpeg's reduced transforms are not implemented", slot, s.scale);
		if (s.pln >= 0)
			return set_err(MIJ_E_STATE, "mij_batch_set_arith: slot %d has a plane request, whose samples are the reference's", slot);
	}
	s.arith = arith;
	return MIJ_OK;
}

extern "C" int mij_batch_slot_out_size(const mij_batch *b, int slot, int *w, int *h)
{
	if (!batch_slot(b, slot, "mij_batch_slot_out_size: bad slot"))
		return MIJ_E_ARG;
	const Slot &s = b->slots[(size_t)slot];
	if (w)
		*w = out_w(s);
	if (h)
		*h = out_h(s);
	return MIJ_OK;
}

/* ---- region of interest (include/mij.h) */

static bool rect_inside(const int r[4], int W, int H) { return r[0] >= 0 && r[1] >= 0 && r[2] > 0 && r[3] > 0 && r[2] <= W - r[0] && r[3] <= H - r[1]; }

extern "C" int mij_batch_set_roi(mij_batch *b, int slot, int x0, int y0, int w, int h)
{
	if (!batch_slot(b, slot, "mij_batch_set_roi: bad slot"))
		return MIJ_E_ARG;
	if (b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_set_roi after mij_batch_upload");
	Slot &s = b->slots[(size_t)slot];
	if (s.desc.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_STATE, "slot %d was rejected by the host stage", slot);
	if (w == 0 && h == 0) {
		s.roi_on = false;
		return MIJ_OK;
	}
	if (s.pln >= 0)
		return set_err(MIJ_E_STATE, "mij_batch_set_roi: slot %d has a plane request, which carries its own window", slot);
	const int r[4] = {x0, y0, w, h};
	if (!rect_inside(r, out_w(s), out_h(s)))
		return set_err(MIJ_E_ARG, "mij_batch_set_roi: region %d,%d %dx%d is empty or outside the %dx%d stored picture of slot %d", x0, y0, w, h, out_w(s), out_h(s), slot);
	if (s.f32 >= 0)
		return set_err(MIJ_E_ARG, "mij_batch_set_roi: slot %d has a float output request; float output of a region is not supported", slot);
	s.roi_on = true;
	memcpy(s.roi, r, sizeof(r));
	return MIJ_OK;
}

extern "C" int mij_batch_set_roi_auto(mij_batch *b, int slot, int on)
{
	if (!batch_slot(b, slot, "mij_batch_set_roi_auto: bad slot"))
		return MIJ_E_ARG;
	if (b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_set_roi_auto after mij_batch_upload");
	Slot &s = b->slots[(size_t)slot];
	if (s.desc.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_STATE, "slot %d was rejected by the host stage", slot);
	if (on && s.pln >= 0)
		return set_err(MIJ_E_STATE, "mij_batch_set_roi_auto: slot %d has a plane request, which carries its own window", slot);
	if (on && s.f32 >= 0)
		return set_err(MIJ_E_ARG, "mij_batch_set_roi_auto: slot %d has a float output request; float output of a region is not supported", slot);
	s.roi_auto = on != 0;
	return MIJ_OK;
}

extern "C" int mij_batch_slot_roi_rect(const mij_batch *b, int slot, int rect[4])
{
	if (!rect || !batch_slot(b, slot))
		return set_err(MIJ_E_ARG, "mij_batch_slot_roi_rect: bad slot or destination");
	if (!b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_slot_roi_rect before mij_batch_upload");
	const Slot &s = b->slots[(size_t)slot];
	if (s.reg) {
		memcpy(rect, s.rect, sizeof(s.rect));
	} else {
		rect[0] = rect[1] = 0;
		rect[2] = out_w(s);
		rect[3] = out_h(s);
	}
	return MIJ_OK;
}

extern "C" int mij_batch_slot_work_items(const mij_batch *b, int slot)
{
	if (!batch_slot(b, slot, "mij_batch_slot_work_items: bad slot"))
		return MIJ_E_ARG;
	if (!b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_slot_work_items before mij_batch_upload");
	return b->slots[(size_t)slot].work_items;
}

extern "C" int mij_batch_slot_kernel(const mij_batch *b, int slot, int *kind, int *variant, int *segments)
{
	if (!batch_slot(b, slot, "mij_batch_slot_kernel: bad slot"))
		return MIJ_E_ARG;
	if (!b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_slot_kernel before mij_batch_upload");
	const Choice &c = b->slots[(size_t)slot].choice;
	if (kind)
		*kind = c.kind;
	if (variant)
		*variant = c.var;
	if (segments)
		*segments = c.nseg;
	return MIJ_OK;
}

/* tests: 1 when the launch that decodes the slot runs the pipelined twin of its kernel (band_prefetch on its list's LDS), 0 when the plain one */
extern "C" int mij_batch_slot_pipelined(const mij_batch *b, int slot)
{
	if (!batch_slot(b, slot, "mij_batch_slot_pipelined: bad slot"))
		return MIJ_E_ARG;
	if (!b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_slot_pipelined before mij_batch_upload");
	const Choice &c = b->slots[(size_t)slot].choice;
	for (const mij_batch::Launch &l : b->launches)
		if (l.kind == c.kind && l.var == c.var)
			return band_prefetch(l.kind, l.var, l.lds, (size_t)b->ctx->max_dyn_lds) ? 1 : 0;
	return 0;
}

/* tests: 1 when that launch runs the twin whose phase B marches down its lanes' own strips (band_march), 0 otherwise */
extern "C" int mij_batch_slot_marched(const mij_batch *b, int slot)
{
	if (!batch_slot(b, slot, "mij_batch_slot_marched: bad slot"))
		return MIJ_E_ARG;
	if (!b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_slot_marched before mij_batch_upload");
	const Choice &c = b->slots[(size_t)slot].choice;
	for (const mij_batch::Launch &l : b->launches)
		if (l.kind == c.kind && l.var == c.var)
			return l.marched ? 1 : 0;
	return 0;
}

extern "C" int mij_batch_set_color(mij_batch *b, int slot, int color)
{
	if (!batch_slot(b, slot))
		return MIJ_E_ARG;
	Slot &s = b->slots[(size_t)slot];
	mij_image_desc d = s.desc;
	d.color = color;
	int rc = check_desc(&d);
	if (rc != MIJ_OK)
		return rc;
	if (s.scale > 1 && scaled_layout(d) < 0)
		return set_err(MIJ_E_ARG, "mij_batch_set_color: slot %d is decoded at 1/%d size, which colour mode %d does not support", slot, s.scale, color);
	if (s.arith == MIJ_ARITH_LIBJPEG && lj_layout(d) < 0)
		return set_err(MIJ_E_ARG, "mij_batch_set_color: slot %d is decoded with libjpeg's arithmetic, which colour mode %d does not support", slot, color);
	s.desc.color = color;
	s.dev.color = color;
	b->uploaded = b->launched = false;
	return MIJ_OK;
}

extern "C" int mij_batch_set_dequant(mij_batch *b, int slot, const mij_image_desc *from)
{
	if (!from || !batch_slot(b, slot))
		return set_err(MIJ_E_ARG, "mij_batch_set_dequant: bad slot or descriptor");
	Slot &s = b->slots[(size_t)slot];
	if (from->ncomp != s.desc.ncomp)
		return set_err(MIJ_E_ARG, "mij_batch_set_dequant: the descriptor has %d components, slot %d has %d", from->ncomp, slot, s.desc.ncomp);
	for (int c = 0; c < s.desc.ncomp; ++c)
		if (from->comp[c].tq < 0 || from->comp[c].tq > 3)
			return set_err(MIJ_E_ARG, "mij_batch_set_dequant: table id %d", from->comp[c].tq);
	/* the slot and the clones made of it so far: they are the same picture (mij_batch_add_clone always names the root) */
	for (size_t i = (size_t)slot; i < b->slots.size(); ++i) {
		Slot &t = b->slots[i];
		if ((int)i != slot && t.clone_of != slot)
			continue;
		for (int c = 0; c < t.desc.ncomp; ++c)
			t.desc.comp[c].tq = from->comp[c].tq;
		memcpy(t.desc.dequant, from->dequant, sizeof(t.desc.dequant));
		fill_dev_dequant(t);
	}
	b->uploaded = b->launched = false;
	return MIJ_OK;
}

extern "C" int mij_batch_image_count(const mij_batch *b) { return b ? (int)b->slots.size() : 0; }
extern "C" int mij_batch_slot_path(const mij_batch *b, int slot)
{
	if (!batch_slot(b, slot))
		return 0;
	return b->slots[(size_t)slot].choice.path;
}
extern "C" int mij_batch_force_generic(mij_batch *b, int on)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	b->force_generic = on < 0 ? 0 : (on > 2 ? 2 : on);
	b->uploaded = b->launched = false;
	return MIJ_OK;
}

/* Which specialised pass 2 (RS_*, mij_kernels.h) serves an image of the two-pass path, or -1 for the run-time-general
 * k_resample_color: component 0 (and 3) at full resolution, components 1 and 2 sharing factors that divide, W % 4 == 0,
 * three or four output channels.  *ycc: YCbCr colour (stbi__YCbCr_to_RGB_row) as opposed to RGB-tagged / CMYK / YCCK. */
static int resample_fast_kind(const mij_batch *b, const mij_image_desc &d, int *ycc)
{
	if (b->force_generic >= 2 || (d.n_out != 3 && d.n_out != 4) || (d.width & 3) || d.ncomp < 3)
		return -1;
	const bool four = d.color == MIJ_COLOR_CMYK || d.color == MIJ_COLOR_YCCK;
	if (d.color != MIJ_COLOR_YCBCR && d.color != MIJ_COLOR_YCBCRA && d.color != MIJ_COLOR_RGB && !four)
		return -1;
	if ((four && d.ncomp != 4) || d.comp[0].h != d.h_max || d.comp[0].v != d.v_max)
		return -1;
	if (four && (d.comp[3].h != d.h_max || d.comp[3].v != d.v_max))
		return -1;
	if (d.comp[1].h != d.comp[2].h || d.comp[1].v != d.comp[2].v || d.h_max % d.comp[1].h || d.v_max % d.comp[1].v)
		return -1;
	const int hs = d.h_max / d.comp[1].h, vs = d.v_max / d.comp[1].v;
	*ycc = (d.color == MIJ_COLOR_YCBCR || d.color == MIJ_COLOR_YCBCRA) ? 1 : 0;
	if (hs == 1)
		return vs == 2 ? RS_V2 : RS_ROW1;
	if (hs == 2)
		return vs == 1 ? RS_H2 : (vs == 2 ? RS_HV2 : RS_GEN2);
	return hs == 4 ? RS_GEN4 : -1;
}

static bool all_1x1(const mij_image_desc &d)
{
	for (int c = 0; c < d.ncomp; ++c)
		if (d.comp[c].h != 1 || d.comp[c].v != 1)
			return false;
	return (uint64_t)d.width * d.height * d.n_out < 0xfffffff0ull;
}

/* LDS per MCU column of the band kernels: 4:2:0, and 4:4:0 (H2 = false) */
static const size_t LDS_COL_420 = 16 * 16 + 2 * 8 * 8 + 2 * 16 + 4 * 8, LDS_COL_440 = 16 * 8 + 2 * 8 * 8 + 2 * 8 + 4 * 8;
/* MCU columns up to which the 4:2:0 and 4:2:2 band kernels run with one / two waves (mij_kernels.h, k_fused420s / t) */
static const int ONE_WAVE_COLS = 24, TWO_WAVE_COLS = 56;

/* Which form of a band kernel a picture takes: by the workgroups of its width that fit a CU's LDS, and for narrow pictures by how many
 * waves a row of MCUs keeps busy (mij_kernels.h, k_fused420w / x / s / t) */
static int band_form(size_t lds, size_t cap, int mcu_x, int mk, int mk_w, int mk_x, int mk_s, int mk_t)
{
	if (2 * lds > cap)
		return mk_x;
	if (3 * lds > cap)
		return mk_w;
	return mcu_x <= ONE_WAVE_COLS ? mk_t : (mcu_x <= TWO_WAVE_COLS ? mk_s : mk);
}

/* Column segments of a picture too wide for one workgroup's LDS (bytes_per_col per MCU column): the fewest segments, of equal width, of
 * which two fit a CU with their two halo columns each.  Returns the segment count; segment k spans MCU columns [mcu_x * k / n, mcu_x * (k + 1) / n). */
static int band_segments(size_t cap, int mcu_x, size_t bytes_per_col)
{
	const int fit = (int)(cap / (2 * bytes_per_col)) - 2; /* two workgroups per CU (mij_kernels.h, k_fused420c) */
	if (fit < 1)
		return mcu_x; /* cannot happen with 160 KiB of LDS: one column per segment */
	return (mcu_x + fit - 1) / fit;
}
static size_t band_segment_lds(int mcu_x, int nseg, size_t bytes_per_col)
{
	int widest = 0;
	for (int k = 0; k < nseg; ++k) {
		const int w = (int)((long)mcu_x * (k + 1) / nseg - (long)mcu_x * k / nseg);
		widest = w > widest ? w : widest;
	}
	return (size_t)(widest + 2) * bytes_per_col;
}

/* The kernel family of a slot, in order of precedence: fused 4:2:0, grey, 4:2:2, 4:4:0, 4:4:4, 1x1 colour, else the two-pass path.
 * The YCbCr band kernels take any width (a row of MCUs beyond the LDS of a CU goes in column segments) but 4:2:2, whose row has to fit. */
static Choice classify(const mij_batch *b, const Slot &s)
{
	const mij_image_desc &d = s.desc;
	const size_t cap = (size_t)b->ctx->max_dyn_lds;
	const int o4 = d.n_out == 4 ? 4 : 0, var = o4 | ((d.flags & MIJ_FLAG_WIDE_IDCT) ? 2 : 0) | (s.coef_bytes_fmt ? 1 : 0);
	if (d.flags & MIJ_FLAG_SKIP) /* rejected by the host stage after it got a slot */
		return Choice();
	if (s.pln >= 0) /* plane output: no pixel kernel, whatever the layout and whatever force_generic says */
		return Choice{PATH_PLANES_OUT, MK_PLANES_OUT, (var & 3) | (b->pln_req[(size_t)s.pln].dev.c[1].form == PLN_PAIRED ? 4 : 0)};
	if (s.arith == MIJ_ARITH_LIBJPEG) /* its own two passes, whatever force_generic says; the variant is pass 2's: n_out - 1 */
		return Choice{PATH_LIBJPEG, MK_LJ_COLOR + lj_layout(d), d.n_out - 1};
	if (s.scale > 1) /* reduced-size decode: one family per layout, whatever force_generic says (the two-pass path has no such form) */
		return Choice{PATH_SCALED, MK_SCALED + scaled_layout(d), (s.scale == 2 ? 0 : (s.scale == 4 ? 2 : 4)) | (s.coef_bytes_fmt ? 1 : 0)};
	if (!b->force_generic) {
		const bool rgb_out = d.n_out == 3 || d.n_out == 4;
		const bool ycc = d.ncomp == 3 && d.color == MIJ_COLOR_YCBCR && rgb_out && d.comp[1].h == 1 && d.comp[1].v == 1 && d.comp[2].h == 1 && d.comp[2].v == 1;
		const int lh = d.comp[0].h, lv = d.comp[0].v;
		/* one component -- or the luma of a YCbCr file asked for as grey (req_comp 1 / 2: the reference resamples only component 0
		 * then, codec/jpeg.c:2246,:2380-2430), when the luma plane has the picture's own resolution: the chroma planes are not even
		 * transformed */
		const bool luma_only = d.ncomp == 3 && lh == d.h_max && lv == d.v_max && d.n_out < 3;
		if (ycc && lh == 2 && lv == 2) {
			const size_t lds = (size_t)d.mcu_x * LDS_COL_420;
			const int mk = lds > cap ? MK_420C : band_form(lds, cap, d.mcu_x, MK_420, MK_420W, MK_420X, MK_420S, MK_420T);
			return Choice{PATH_420, mk, var, mk == MK_420C ? band_segments(cap, d.mcu_x, LDS_COL_420) : 1, lds};
		}
		if ((d.ncomp == 1 || luma_only) && d.color == MIJ_COLOR_GREY && d.n_out >= 1 && d.n_out <= 4 && (uint64_t)d.width * d.height * d.n_out < 0xfffffff0ull)
			return Choice{PATH_GREY, MK_GREY, var & 3};
		if (ycc && lh == 2 && lv == 1 && (size_t)d.mcu_x * 256 + 16 <= cap) {
			const size_t lds = (size_t)d.mcu_x * 256 + 16;
			return Choice{PATH_422, band_form(lds, cap, d.mcu_x, MK_422, MK_422W, MK_422X, MK_422S, MK_422T), var, 1, lds};
		}
		if (ycc && lh == 1 && lv == 2) {
			const size_t lds = (size_t)d.mcu_x * LDS_COL_440;
			const int mk = lds > cap ? MK_440C : (3 * lds > cap ? MK_440W : MK_440);
			return Choice{PATH_440, mk, var, mk == MK_440C ? band_segments(cap, d.mcu_x, LDS_COL_440) : 1, lds};
		}
		/* 4:4:4: three-component YCbCr, or four components whose transform is YCbCr with the fourth ignored (codec/jpeg.c:2367-2370): the
		 * kernel only touches components 0-2.  k_fused1x1c: RGB-tagged (codec/jpeg.c:2325-2335), Adobe CMYK (:2343-2354), YCCK (:2355-2366) */
		if (rgb_out && ((d.ncomp == 3 && d.color == MIJ_COLOR_YCBCR) || (d.ncomp == 4 && d.color == MIJ_COLOR_YCBCRA)) && all_1x1(d))
			return Choice{PATH_444, MK_444, var};
		if (rgb_out && ((d.ncomp == 3 && d.color == MIJ_COLOR_RGB) || (d.ncomp == 4 && (d.color == MIJ_COLOR_CMYK || d.color == MIJ_COLOR_YCCK))) && all_1x1(d))
			return Choice{PATH_1X1C, MK_1X1C, var};
	}
	int ycc = 0;
	const int rk = resample_fast_kind(b, d, &ycc);
	return rk < 0 ? Choice{PATH_TWO_PASS, MK_RESAMPLE, 0} : Choice{PATH_TWO_PASS, MK_RS_FAST + rk, o4 | ycc << 1};
}

/* Small tables (image descriptors, work lists, Huffman tables) go to the device by a copy KERNEL reading the
 * pinned host buffer, not by hipMemcpyAsync: with several batches in flight the runtime's copy path made the host
 * wait behind other streams' large transfers (measured: 8 ms for a 100 KB copy, one call in four).  Sizes are
 * multiples of 4; the buffers come from hipHostMalloc, which maps them for the device. */
__global__ __launch_bounds__(256) void k_copy_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src, uint32_t n)
{
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
		dst[i] = src[i];
}

__global__ __launch_bounds__(256) void k_copy_words16(uint4 *__restrict__ dst, const uint4 *__restrict__ src, uint32_t n)
{
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
		dst[i] = src[i];
}

static hipError_t copy_table(void *dst, const void *src_pinned, size_t bytes, hipStream_t st)
{
	void *dsrc = nullptr;
	if (bytes == 0)
		return hipSuccess;
	if ((bytes & 3u) || bytes > (1u << 30) || hipHostGetDevicePointer(&dsrc, const_cast<void *>(src_pinned), 0) != hipSuccess || !dsrc) {
		(void)hipGetLastError();
		return hipMemcpyAsync(dst, src_pinned, bytes, hipMemcpyHostToDevice, st);
	}
	if (!((uintptr_t)dst & 15u) && !((uintptr_t)dsrc & 15u) && !(bytes & 15u) && bytes >= 65536) { /* the entropy streams: tens of MB */
		const uint32_t n = (uint32_t)(bytes / 16);
		const unsigned grid = (n + 1023u) / 1024u > 512u ? 512u : (n + 1023u) / 1024u;
		hipLaunchKernelGGL(k_copy_words16, dim3(grid ? grid : 1u), dim3(256), 0, st, static_cast<uint4 *>(dst), static_cast<const uint4 *>(dsrc), n);
		return hipGetLastError();
	}
	const uint32_t n = (uint32_t)(bytes / 4);
	const unsigned grid = (n + 1023u) / 1024u > 1024u ? 1024u : (n + 1023u) / 1024u;
	hipLaunchKernelGGL(k_copy_words, dim3(grid ? grid : 1u), dim3(256), 0, st, static_cast<uint32_t *>(dst), static_cast<const uint32_t *>(dsrc), n);
	return hipGetLastError();
}

/* the other direction for small results (verdict words): the kernel writes the pinned host buffer through its device mapping */
static hipError_t copy_table_to_host(void *dst_pinned, const void *src_dev, size_t bytes, hipStream_t st)
{
	void *ddst = nullptr;
	if (bytes == 0)
		return hipSuccess;
	if ((bytes & 3u) || hipHostGetDevicePointer(&ddst, dst_pinned, 0) != hipSuccess || !ddst) {
		(void)hipGetLastError();
		return hipMemcpyAsync(dst_pinned, src_dev, bytes, hipMemcpyDeviceToHost, st);
	}
	const uint32_t n = (uint32_t)(bytes / 4);
	const unsigned grid = (n + 1023u) / 1024u > 1024u ? 1024u : (n + 1023u) / 1024u;
	hipLaunchKernelGGL(k_copy_words, dim3(grid ? grid : 1u), dim3(256), 0, st, static_cast<uint32_t *>(ddst), static_cast<const uint32_t *>(src_dev), n);
	return hipGetLastError();
}

/* Puts an output pass's plan of `need` bytes on the device: grows the buffer (Grow waits for the stream first, whose launches may
 * still read the old one), lets fill write the pinned side, copies it up on the batch stream, and records the items and offsets. */
template <typename Fill>
static int plan_put(mij_batch *b, PlanBuf &p, size_t need, size_t items, size_t lut_at, size_t work_at, Fill fill)
{
	Grow grow(b->stream);
	grow(p.buf, align_up(need, 4));
	if (grow.rc != MIJ_OK)
		return grow.rc;
	fill(p.buf.h);
	HIP_TRY(copy_table(p.buf.d, p.buf.h, align_up(need, 4), b->stream));
	p.items = items;
	p.lut_at = lut_at;
	p.work_at = work_at;
	return MIJ_OK;
}

/* Float output: k_out_f32's descriptors, tables and work list -- (float slot, chunk) items, MIJ_F32_CHUNK input bytes each -- built
 * next to the decode plan and copied up on the batch stream.  A batch without float requests does nothing here. */
static int f32_plan(mij_batch *b)
{
	b->f32plan.items = 0;
	const size_t nreq = b->f32_req.size();
	if (!nreq)
		return MIJ_OK;
	std::vector<WorkF32> work;
	for (size_t f = 0; f < nreq; ++f) {
		const Slot &s = b->slots[(size_t)b->f32_req[f].slot];
		if (s.desc.flags & MIJ_FLAG_SKIP)
			continue;
		const uint64_t nbytes = (uint64_t)s.desc.n_out * (uint64_t)s.desc.width * (uint64_t)s.desc.height;
		for (uint64_t c = 0; c * MIJ_F32_CHUNK < nbytes; ++c)
			work.push_back(WorkF32{(uint32_t)f, (uint32_t)c});
	}
	if (work.empty())
		return MIJ_OK;
	const size_t lut_at = align_up(sizeof(DevF32) * nreq, 256), work_at = lut_at + sizeof(float) * MIJ_F32_LUT_FLOATS * nreq;
	const size_t need = work_at + sizeof(WorkF32) * work.size();
	return plan_put(b, b->f32plan, need, work.size(), lut_at, work_at, [&](uint8_t *h) {
		DevF32 *fd = reinterpret_cast<DevF32 *>(h);
		for (size_t f = 0; f < nreq; ++f) {
			const mij_batch::F32Req &q = b->f32_req[f];
			const Slot &s = b->slots[(size_t)q.slot];
			fd[f].src_off = s.dev.out_off;
			fd[f].dst_off = q.off;
			fd[f].nbytes = (uint64_t)s.desc.n_out * (uint64_t)s.desc.width * (uint64_t)s.desc.height;
			fd[f].n_out = (uint32_t)s.desc.n_out;
			fd[f].pad = 0;
			memcpy(h + lut_at + sizeof(float) * MIJ_F32_LUT_FLOATS * f, q.lut, sizeof(q.lut));
		}
		memcpy(h + work_at, work.data(), sizeof(WorkF32) * work.size());
	});
}

/* k_out_tensor's / k_out_resize's descriptor of a request */
static void dev_tensor(DevTensor &d, const mij_batch::TenReq &q, const Slot &s)
{
	d.src_off = s.dev.out_off;
	d.dst = (uint64_t)(uintptr_t)q.t.dst;
	d.row_pitch = q.t.row_pitch;
	d.plane_pitch = q.t.layout == MIJ_LAYOUT_CHW ? q.t.plane_pitch : 0;
	d.src_w = (uint32_t)out_w(s);
	d.n_out = (uint32_t)s.desc.n_out;
	d.x0 = (uint32_t)q.t.x0;
	d.y0 = (uint32_t)q.t.y0;
	d.w = (uint32_t)q.t.w;
	d.h = (uint32_t)q.t.h;
	d.flip_x = q.t.flip_x ? 1u : 0u;
	d.flip_y = q.t.flip_y ? 1u : 0u;
	d.esize = q.esize;
	d.chw = q.t.layout == MIJ_LAYOUT_CHW ? 1u : 0u;
	d.lut = q.lut ? 1u : 0u;
	d.pad = 0;
}

/* Tensor output: k_out_tensor's descriptors, tables and work list -- (request, band of window rows, segment of window columns) items of
 * at most MIJ_TEN_ITEM_BYTES source bytes and MIJ_TEN_MAX_ROWS rows -- built next to the decode plan and copied up on the batch stream.
 * With tr, k_out_tensor_t's for the transposed requests instead: tiles of at most MIJ_TEN_TR_BYTES bytes of each of at most
 * MIJ_TEN_STAGE_WORDS / pitch stored-row segments, near square in pixels.  A batch without such requests does nothing here. */
#define MIJ_TEN_TR_BYTES 192u
static int ten_plan(mij_batch *b, bool tr)
{
	PlanBuf &pb = tr ? b->tentplan : b->tenplan;
	pb.items = 0;
	const size_t nreq = b->ten_req.size();
	if (!nreq)
		return MIJ_OK;
	std::vector<WorkTensor> work;
	for (size_t t = 0; t < nreq; ++t) {
		const mij_batch::TenReq &q = b->ten_req[t];
		if ((b->slots[(size_t)q.slot].desc.flags & MIJ_FLAG_SKIP) || q.rsz || q.tr != tr) /* resized requests: rsz_plan */
			continue;
		const uint32_t c = (uint32_t)b->slots[(size_t)q.slot].desc.n_out, w = (uint32_t)q.t.w, h = (uint32_t)q.t.h;
		if (tr) {
			const uint32_t rows = std::min(h, std::max(1u, MIJ_TEN_TR_BYTES / c)), lsd = ((rows * c + 3u) >> 2) | 1u;
			const uint32_t cols = std::min(w, MIJ_TEN_STAGE_WORDS / lsd);
			for (uint32_t r0 = 0; r0 < h; r0 += rows)
				for (uint32_t p0 = 0; p0 < w; p0 += cols)
					work.push_back(WorkTensor{(uint32_t)t, r0, p0, (uint16_t)std::min(rows, h - r0), (uint16_t)std::min(cols, w - p0)});
			continue;
		}
		const uint32_t segw = std::min(w, MIJ_TEN_ITEM_BYTES / c);
		for (uint32_t p0 = 0; p0 < w; p0 += segw) {
			const uint32_t np = std::min(segw, w - p0);
			const uint32_t rows = std::max(1u, std::min(std::min(h, MIJ_TEN_MAX_ROWS), MIJ_TEN_ITEM_BYTES / (np * c)));
			for (uint32_t r0 = 0; r0 < h; r0 += rows)
				work.push_back(WorkTensor{(uint32_t)t, r0, p0, (uint16_t)std::min(rows, h - r0), (uint16_t)np});
		}
	}
	if (work.empty())
		return MIJ_OK;
	if (work.size() > 0x7fffffffu)
		return set_err(MIJ_E_ARG, "tensor output: %zu work items", work.size());
	const size_t lut_at = align_up(sizeof(DevTensor) * nreq, 256), work_at = lut_at + MIJ_TEN_LUT_BYTES * nreq;
	const size_t need = work_at + sizeof(WorkTensor) * work.size();
	return plan_put(b, pb, need, work.size(), lut_at, work_at, [&](uint8_t *h) {
		DevTensor *td = reinterpret_cast<DevTensor *>(h);
		for (size_t t = 0; t < nreq; ++t) {
			const mij_batch::TenReq &q = b->ten_req[t];
			dev_tensor(td[t], q, b->slots[(size_t)q.slot]);
			memcpy(h + lut_at + MIJ_TEN_LUT_BYTES * t, q.table, MIJ_TEN_LUT_BYTES);
		}
		memcpy(h + work_at, work.data(), sizeof(WorkTensor) * work.size());
	});
}

/* Resized tensor output: k_out_resize's descriptors, tables, coefficients (each (in, out, filter) once) and work list -- (request, band of
 * at most MIJ_RSZ_ROWS output rows, segment of output columns) -- in one buffer pair.  A segment has at most one column per lane
 * (256 / n_out), few enough that its horizontal taps fit MIJ_RSZ_KCAP (else they stay in the plan) and, where it can, that its span of
 * source bytes fills at most half the stage, so that a round stages two rows or more.  A band has as many rows as keep its vertical taps
 * within MIJ_RSZ_VCAP (else they stay in the plan).  With tr, k_out_resize_t's plan for the transposed requests, whose span is one of
 * stored rows: where it can, few enough that a round stages 8 stored columns or more.  A batch without such requests does nothing. */
static int rsz_plan(mij_batch *b, bool tr)
{
	PlanBuf &pb = tr ? b->rsztplan : b->rszplan;
	pb.items = 0;
	const size_t nreq = b->ten_req.size();
	size_t nrsz = 0;
	for (const mij_batch::TenReq &q : b->ten_req)
		nrsz += q.rsz && q.tr == tr && !(b->slots[(size_t)q.slot].desc.flags & MIJ_FLAG_SKIP);
	if (!nrsz)
		return MIJ_OK;
	/* byte offsets of the coefficient blocks, each (in, out, filter) once */
	std::map<const mij_batch::RszCoef *, uint64_t> at;
	const size_t lut_at = align_up(sizeof(DevResize) * nreq, 256), coef_at = lut_at + MIJ_TEN_LUT_BYTES * nreq;
	size_t off = coef_at;
	std::vector<WorkResize> work;
	std::vector<uint32_t> kglobal(nreq, 0), vglobal(nreq, 0);
	for (size_t t = 0; t < nreq; ++t) {
		const mij_batch::TenReq &q = b->ten_req[t];
		if (!q.rsz || q.tr != tr || (b->slots[(size_t)q.slot].desc.flags & MIJ_FLAG_SKIP))
			continue;
		for (const mij_batch::RszCoef *c : {q.ch, q.cv})
			if (at.emplace(c, off).second)
				off += c->v.size() * sizeof(int32_t);
		const uint32_t n = (uint32_t)b->slots[(size_t)q.slot].desc.n_out, ow = (uint32_t)q.r.out_w, oh = (uint32_t)q.r.out_h;
		const uint32_t ksh = (uint32_t)q.ch->ks;
		uint32_t nc = 256u / n;
		if (ksh > MIJ_RSZ_KCAP)
			kglobal[t] = 1;
		else
			nc = std::min(nc, MIJ_RSZ_KCAP / ksh);
		/* source columns in half the stage; transposed, stored rows of which the stage holds 8 columns */
		const double scale = (double)q.t.w / ow, half = tr ? (double)MIJ_RSZ_STAGE_WORDS / (((8u * n + 3u) >> 2) | 1u) : MIJ_RSZ_STAGE_WORDS * 2.0 / n;
		if ((nc * scale + ksh) > half)
			nc = (uint32_t)std::max(1.0, std::min((double)nc, (half - ksh) / scale));
		const uint32_t nseg = (ow + nc - 1) / nc, segw = (ow + nseg - 1) / nseg;
		const uint32_t ksv = (uint32_t)q.cv->ks, rows = ksv > MIJ_RSZ_VCAP ? MIJ_RSZ_ROWS : std::min(MIJ_RSZ_ROWS, MIJ_RSZ_VCAP / ksv);
		vglobal[t] = ksv > MIJ_RSZ_VCAP ? 1u : 0u;
		const uint32_t nband = (oh + rows - 1) / rows, bandh = (oh + nband - 1) / nband;
		for (uint32_t q0 = 0; q0 < oh; q0 += bandh)
			for (uint32_t u0 = 0; u0 < ow; u0 += segw)
				work.push_back(WorkResize{(uint32_t)t, q0, u0, (uint16_t)std::min(bandh, oh - q0), (uint16_t)std::min(segw, ow - u0)});
	}
	if (work.size() > 0x7fffffffu)
		return set_err(MIJ_E_ARG, "resized tensor output: %zu work items", work.size());
	const size_t work_at = align_up(off, 16), need = work_at + sizeof(WorkResize) * work.size();
	return plan_put(b, pb, need, work.size(), lut_at, work_at, [&](uint8_t *h) {
		DevResize *rd = reinterpret_cast<DevResize *>(h);
		memset(rd, 0, sizeof(DevResize) * nreq);
		for (size_t t = 0; t < nreq; ++t) {
			const mij_batch::TenReq &q = b->ten_req[t];
			if (!q.rsz || q.tr != tr || (b->slots[(size_t)q.slot].desc.flags & MIJ_FLAG_SKIP))
				continue;
			DevResize &d = rd[t];
			dev_tensor(d.t, q, b->slots[(size_t)q.slot]);
			d.hco = at[q.ch];
			d.vco = at[q.cv];
			d.out_w = (uint32_t)q.r.out_w;
			d.out_h = (uint32_t)q.r.out_h;
			d.ksh = (uint32_t)q.ch->ks;
			d.ksv = (uint32_t)q.cv->ks;
			d.mul32 = (q.ch->big || q.cv->big) ? 1u : 0u;
			d.kglobal = kglobal[t];
			d.vglobal = vglobal[t];
			memcpy(h + lut_at + MIJ_TEN_LUT_BYTES * t, q.table, MIJ_TEN_LUT_BYTES);
		}
		for (const auto &e : at)
			memcpy(h + e.second, e.first->v.data(), e.first->v.size() * sizeof(int32_t));
		memcpy(h + work_at, work.data(), sizeof(WorkResize) * work.size());
	});
}

/* ---- mij_batch_upload, step by step.  Each step keeps its copies and launches on the batch stream in the order given here. */

static bool host_staged(const Slot &s) { return s.clone_of < 0 && !s.dev_coef; }
static bool l1_on_device(const Slot &s) { return host_staged(s) && (s.desc.flags & MIJ_FLAG_L1_ON_DEVICE) && !(s.desc.flags & MIJ_FLAG_SKIP); }

/* (slot, component, first block) per 256 blocks of a component's tiles: the pack kernel's work items */
static void push_tiles(std::vector<Work4> &L, uint32_t i, const mij_image_desc &d)
{
	for (int c = 0; c < d.ncomp; ++c)
		for (uint32_t f = 0, nb = (uint32_t)comp_tiles(d.comp[c]) * 64u; f < nb; f += 256)
			L.push_back(Work4{i, (uint32_t)c, f, 0u});
}

/* Format of the planes in HBM.  Slots the GPU entropy stage wrote keep theirs; host-staged slots get the batch's format (compact by
 * default: uploaded as int16 into the scratch, packed by k_pack_c8); clones follow their source (which precedes them). */
static int plane_formats(mij_batch *b)
{
	bool need_pack = false;
	for (Slot &s : b->slots) {
		if (s.clone_of >= 0)
			s.coef_bytes_fmt = b->slots[(size_t)s.clone_of].coef_bytes_fmt;
		else if (!s.dev_coef) /* planes the host staged compact keep that format whatever the batch's default */
			s.coef_bytes_fmt = ((b->coef_fmt || (s.desc.flags & (MIJ_FLAG_STAGED_COMPACT | MIJ_FLAG_L1_ON_DEVICE))) && !(s.desc.flags & MIJ_FLAG_SKIP)) ? 1 : 0;
		layout_coef(s);
		if (host_staged(s) && s.coef_bytes_fmt && !(s.desc.flags & MIJ_FLAG_STAGED_COMPACT))
			need_pack = true;
	}
	if (need_pack && !b->up16.d) {
		hipError_t e = b->up16.alloc(b->stage.cap);
		if (e != hipSuccess)
			return set_err(e == hipErrorOutOfMemory ? MIJ_E_NOMEM : MIJ_E_HIP, "upload scratch: %s", hipGetErrorString(e));
	}
	return MIJ_OK;
}

/* Progressive files whose L1 bound the host left to the device (MIJ_FLAG_L1_ON_DEVICE): their planes go up and are packed NOW, the
 * pack kernel takes every block's L1 on the way, the maxima come back, and MIJ_FLAG_WIDE_IDCT is set before the decode plan sorts the
 * images by it.  Afterwards these slots hold finished compact planes in HBM (dev_coef: later uploads leave them alone). */
static int l1_prepack(mij_batch *b)
{
	const size_t n = b->slots.size();
	std::vector<Work4> pre;
	for (size_t i = 0; i < n; ++i)
		if (l1_on_device(b->slots[i]))
			push_tiles(pre, (uint32_t)i, b->slots[i].desc);
	if (pre.empty())
		return MIJ_OK;
	if (!b->l1max.cap) /* a failure leaves cap 0: the next upload tries again */
		HIP_TRY(b->l1max.alloc((size_t)b->max_images));
	Grow grow(b->stream);
	grow(b->work, pre.size());
	if (grow.rc != MIJ_OK)
		return grow.rc;
	memcpy(b->work.h, pre.data(), pre.size() * sizeof(Work4));
	for (size_t i = 0; i < n; ++i) {
		Slot &s = b->slots[i];
		s.dev.src16_off = s.stage_off == MIJ_NO_STAGE ? 0 : s.stage_off;
		b->imgs.h[i] = s.dev;
		if (host_staged(s) && (s.desc.flags & MIJ_FLAG_L1_ON_DEVICE))
			b->imgs.h[i].flags |= MIJ_DEV_L1_MAX;
	}
	HIP_TRY(copy_table(b->imgs.d, b->imgs.h, sizeof(DevImage) * n, b->stream));
	HIP_TRY(copy_table(b->work.d, b->work.h, sizeof(Work4) * pre.size(), b->stream));
	HIP_TRY(hipMemsetAsync(b->l1max.d, 0, sizeof(uint32_t) * n, b->stream));
	for (const Slot &s : b->slots)
		if (l1_on_device(s)) {
			size_t bytes16 = 0;
			for (int c = 0; c < s.desc.ncomp; ++c)
				bytes16 += comp_tiles(s.desc.comp[c]) << 13;
			HIP_TRY(hipMemcpyAsync(b->up16.d + s.stage_off, b->stage.h + s.stage_off, bytes16, hipMemcpyHostToDevice, b->stream));
		}
	hipLaunchKernelGGL(k_pack_c8, dim3((unsigned)pre.size()), dim3(256), 0, b->stream, b->imgs.d, reinterpret_cast<const WorkIdct *>(b->work.d), b->up16.d, b->coef.d, b->l1max.d);
	HIP_TRY(hipGetLastError());
	HIP_TRY(copy_table_to_host(b->l1max.h, b->l1max.d, sizeof(uint32_t) * n, b->stream));
	HIP_TRY(hipStreamSynchronize(b->stream));
	for (size_t i = 0; i < n; ++i) {
		Slot &s = b->slots[i];
		if (l1_on_device(s)) {
			s.desc.flags &= ~(uint32_t)MIJ_FLAG_L1_ON_DEVICE;
			if (b->l1max.h[i] > (uint32_t)MIJ_BLOCK_L1_LIMIT)
				s.desc.flags |= MIJ_FLAG_WIDE_IDCT;
			s.dev.flags = (int32_t)s.desc.flags | MIJ_DEV_COEF_BYTES;
			s.dev_coef = 1;
		}
	}
	for (Slot &s : b->slots) /* clones take their source's verdict */
		if (s.clone_of >= 0 && (s.desc.flags & MIJ_FLAG_L1_ON_DEVICE)) {
			s.desc.flags = b->slots[(size_t)s.clone_of].desc.flags;
			s.dev.flags = (int32_t)s.desc.flags | MIJ_DEV_COEF_BYTES;
		}
	return MIJ_OK;
}

/* The decode plan: one work list per (kernel family, variant) with the LDS its launch needs, the pack list, and the bytes of scratch
 * sample planes the two-pass path needs */
namespace {
struct Plan {
	std::vector<Work4> pack, lists[MK_KINDS][MK_VARIANTS];
	size_t lds[MK_KINDS][MK_VARIANTS] = {};
	size_t planes_need = 0;
};
} // namespace

/* Automatic band count per family of the 4:2:0 / 4:4:0 band kernels.  The grid runs in "rounds" of (CUs x workgroups per CU by LDS)
 * co-resident workgroups; the last round of a launch is only as full as the remainder, and every band re-does two chroma block rows
 * of IDCT as halo.  Pick the bands-per-image (1..16) that minimises  rounds x (1 + halo share)  per unit of work; measured on MI355X:
 * 1024 x 1080p -> 6 bands (6144 workgroups = 8.0 rounds of 768) beats 4 (5.33 rounds) by ~1.5 %. */
static const int BAND_CAP = 64; /* most bands per picture of a small 4:2:0 batch, below */
static void auto_bands(const mij_batch *b, int nb[MK_KINDS])
{
	size_t n_fused[MK_KINDS] = {}, mcu_rows_sum[MK_KINDS] = {}, lds_max[MK_KINDS] = {};
	for (const Slot &s : b->slots)
		if ((s.choice.path == PATH_420 || s.choice.path == PATH_440) && !s.reg) { /* a slot with a region cuts its own bands (push_region_bands) */
			const int k = s.choice.kind;
			++n_fused[k];
			mcu_rows_sum[k] += (size_t)s.desc.mcu_y;
			lds_max[k] = s.choice.lds > lds_max[k] ? s.choice.lds : lds_max[k];
		}
	const int cu = b->ctx->prop.multiProcessorCount > 0 ? b->ctx->prop.multiProcessorCount : 256;
	for (int kind = 0; kind < MK_KINDS; ++kind) {
		nb[kind] = 1;
		if (!n_fused[kind])
			continue;
		size_t per_cu = lds_max[kind] ? (size_t)b->ctx->max_dyn_lds / lds_max[kind] : 1;
		/* waves per SIMD by registers x four SIMDs.  The pipelined twins of MK_420 (k_fused420p, k_fused420m) allow MIJ_F420P_WAVES only, but are taken just where the LDS
		 * bound above is at most that many workgroups of four waves already (band_prefetch), so the count below is right for it as well */
		const size_t by_waves = 4 * MIJ_F420_WAVES / ((size_t)families[kind].threads / 64);
		per_cu = per_cu < 1 ? 1 : (per_cu > by_waves ? by_waves : per_cu);
		const size_t slots = (size_t)cu * per_cu;
		const double avg_rows = (double)mcu_rows_sum[kind] / (double)n_fused[kind];
		double best = 1e30;
		/* up to 16 bands per picture; up to BAND_CAP for 4:2:0 batches so small that sixteen bands each leave workgroup slots
		 * empty (a lone picture from stbi_load, a handful): 16 x 1080p 0.078 -> 0.058 ms.  Not for 4:4:0, whose halo is a larger share
		 * of a band (0.069 -> 0.093 ms), and not once the slots are full (36 x 5120 x 2880: 0.70 -> 0.73 ms with the higher cap). */
		const int cap = (kind != MK_440 && kind != MK_440W && kind != MK_440C && n_fused[kind] * 16 <= slots) ? BAND_CAP : 16;
		for (int k = 1; k <= cap && k <= (int)avg_rows; ++k) {
			const size_t wgs = n_fused[kind] * (size_t)k;
			const size_t rounds = (wgs + slots - 1) / slots;
			/* every inner band edge re-transforms two chroma block rows (4 of an MCU row's 6 blocks' worth), the IDCT being ~45 %
			 * of the work; a launch also pays about 0.3 band lengths of ramp-up and tail whatever its shape -- without that term
			 * the model took 3 bands for 1024 x 1080p where 6 measure 1.5 % faster, and 3 for 256 images where 12 measure 4 % faster
			 * (interleaved runs, profiles/r02z_band_count.txt) */
			const double halo = 1.0 + 0.45 * 4.0 * (k - 1) / (6.0 * avg_rows);
			const double cost = ((double)rounds + 0.3) * (avg_rows / k) * halo; /* time ~ (rounds + ramp) x band length */
			if (cost < best * 0.999) {
				best = cost;
				nb[kind] = k;
			}
		}
	}
}

/* The work items of a 4:2:0 / 4:4:0 picture: nb bands of about equal MCU rows, each split into the choice's column segments of about equal
 * MCU columns (only the column-segmented forms read them), and the LDS they need */
static void push_bands(std::vector<Work4> &L, size_t &lds, uint32_t i, const mij_image_desc &d, const Choice &c, int nb)
{
	nb = nb > d.mcu_y ? d.mcu_y : (nb < 1 ? 1 : nb);
	for (int k = 0; k < nb; ++k)
		for (int g = 0; g < c.nseg; ++g)
			L.push_back(Work4{i, (uint32_t)((long)d.mcu_y * k / nb), (uint32_t)((long)d.mcu_y * (k + 1) / nb),
									(uint32_t)((long)d.mcu_x * g / c.nseg) | (uint32_t)((long)d.mcu_x * (g + 1) / c.nseg) << 16});
	const size_t need = (c.kind == MK_420C || c.kind == MK_440C) ? band_segment_lds(d.mcu_x, c.nseg, c.lds / (size_t)d.mcu_x) : c.lds;
	lds = need > lds ? need : lds;
}

/* The same for a slot with a region: bands over the MCU rows [r0, r1) only, each cut into the fewest column segments of [c0, c1) that fit the
 * LDS as band_segments counts it.  Bands of about four MCU rows: a window is narrow, so a band's workgroup is short of lanes whatever its
 * height, and it is the number of workgroups that fills the machine; the halo a band edge re-transforms is two chroma block rows of the
 * window's width only. */
static void push_region_bands(std::vector<Work4> &L, size_t &lds, uint32_t i, size_t cap, size_t bytes_per_col, int r0, int r1, int c0, int c1, int band_rows)
{
	const int rows = r1 - r0, cols = c1 - c0, nseg = band_segments(cap, cols, bytes_per_col);
	const int per = band_rows > 0 ? band_rows : 4, nb = (rows + per - 1) / per;
	for (int k = 0; k < nb; ++k)
		for (int g = 0; g < nseg; ++g)
			L.push_back(Work4{i, (uint32_t)(r0 + (long)rows * k / nb), (uint32_t)(r0 + (long)rows * (k + 1) / nb),
									(uint32_t)(c0 + (long)cols * g / nseg) | (uint32_t)(c0 + (long)cols * (g + 1) / nseg) << 16});
	const size_t need = band_segment_lds(cols, nseg, bytes_per_col);
	lds = need > lds ? need : lds;
}

/* (slot, first unit) per 256 lane units of a window (the windowed 1 x 1 and reduced-size kernels) */
static void push_window(std::vector<Work4> &L, uint32_t i, const DevRoi &w)
{
	for (uint32_t f = 0, n = w.w * w.h; f < n; f += 256)
		L.push_back(Work4{i, 0u, f, 0u});
}

/* The regions of an upload.  Per slot that asked for one: the region in force -- the explicit one, validated against the stored picture as
 * it is now, or the tensor request's window in the stored frame -- and the checks that tie a request to it. */
static int resolve_regions(mij_batch *b)
{
	for (size_t i = 0; i < b->slots.size(); ++i) {
		Slot &s = b->slots[i];
		s.reg = false;
		if (!wants_region(s) || (s.desc.flags & MIJ_FLAG_SKIP))
			continue;
		int win[4] = {0, 0, 0, 0}; /* the request's window in stored pixels: a transposed request's rows are stored columns */
		if (s.ten >= 0) {
			const mij_batch::TenReq &q = b->ten_req[(size_t)s.ten];
			win[0] = q.t.x0, win[1] = q.t.y0, win[2] = q.tr ? q.t.h : q.t.w, win[3] = q.tr ? q.t.w : q.t.h;
		}
		if (s.roi_on) { /* an explicit region wins over the automatic one */
			if (!rect_inside(s.roi, out_w(s), out_h(s)))
				return set_err(MIJ_E_ARG, "mij_batch_upload: region %d,%d %dx%d of slot %zu is outside its %dx%d stored picture", s.roi[0], s.roi[1], s.roi[2], s.roi[3], i,
									out_w(s), out_h(s));
			if (s.ten >= 0 && (win[0] < s.roi[0] || win[1] < s.roi[1] || win[0] + win[2] > s.roi[0] + s.roi[2] || win[1] + win[3] > s.roi[1] + s.roi[3]))
				return set_err(MIJ_E_ARG, "mij_batch_upload: the tensor request of slot %zu reads %d,%d %dx%d of the stored picture, outside the slot's region %d,%d %dx%d", i,
									win[0], win[1], win[2], win[3], s.roi[0], s.roi[1], s.roi[2], s.roi[3]);
			memcpy(s.reg_px, s.roi, sizeof(s.roi));
		} else {
			if (s.ten < 0)
				return set_err(MIJ_E_STATE, "mij_batch_upload: slot %zu asks for an automatic region (mij_batch_set_roi_auto) but has no tensor request", i);
			memcpy(s.reg_px, win, sizeof(win));
		}
		if (s.f32 >= 0)
			return set_err(MIJ_E_ARG, "mij_batch_upload: slot %zu has a float output request and a region", i);
		s.reg = true;
	}
	return MIJ_OK;
}

/* What a region makes of a slot's choice: the lane-unit rectangle that covers it (MCUs of the band kernels; 8 x 8 blocks of the 1 x 1
 * kernels; MCUs, or luma blocks, of the reduced-size kernels), the decoded rectangle, and the windowed family.  The region is dropped
 * (s.reg = false: the slot is planned as without one) for the two-pass path, which has no windowed form, and when it needs every unit. */
static void apply_region(Slot &s)
{
	const mij_image_desc &d = s.desc;
	Choice &c = s.choice;
	int uw, uh; /* unit size in stored pixels */
	switch (c.path) {
	case PATH_420: uw = 16, uh = 16; break;
	case PATH_440: uw = 8, uh = 16; break;
	case PATH_422: uw = 16, uh = 8; break;
	case PATH_GREY:
	case PATH_444:
	case PATH_1X1C: uw = uh = 8; break;
	case PATH_SCALED: {
		const int lay = c.kind - MK_SCALED, n = 8 / s.scale;
		uw = n * ((lay == SC_420 || lay == SC_422) ? 2 : 1), uh = n * (lay == SC_420 ? 2 : 1);
		break;
	}
	default:
		s.reg = false;
		return;
	}
	const int W = out_w(s), H = out_h(s);
	int x0 = s.reg_px[0] / uw, x1 = (s.reg_px[0] + s.reg_px[2] + uw - 1) / uw, y0 = s.reg_px[1] / uh, y1 = (s.reg_px[1] + s.reg_px[3] + uh - 1) / uh;
	if (c.path == PATH_422) /* rows only: a column form needs the h2v1 filter's halo and edge forms in segments */
		x0 = 0, x1 = d.mcu_x;
	/* the grid may reach beyond the picture (padding MCUs, blocks of a luma plane that no pixel row reads): units that hold pixels only */
	const int ux = (W + uw - 1) / uw, uy = (H + uh - 1) / uh;
	if (x0 == 0 && y0 == 0 && x1 >= ux && y1 >= uy) {
		s.reg = false;
		return;
	}
	s.win = DevRoi{(uint32_t)x0, (uint32_t)y0, (uint32_t)(x1 - x0), (uint32_t)(y1 - y0)};
	s.rect[0] = x0 * uw, s.rect[1] = y0 * uh;
	s.rect[2] = (x1 * uw < W ? x1 * uw : W) - s.rect[0], s.rect[3] = (y1 * uh < H ? y1 * uh : H) - s.rect[1];
	switch (c.path) {
	case PATH_420: c.kind = MK_420C; break;
	case PATH_440: c.kind = MK_440C; break;
	case PATH_444: c.kind = MK_444R; break;
	case PATH_GREY: c.kind = MK_GREYR; break;
	case PATH_1X1C: c.kind = MK_1X1CR; break;
	case PATH_SCALED: c.kind = MK_SCALEDR + (c.kind - MK_SCALED); break;
	default: break; /* PATH_422: the same kernel on fewer bands */
	}
}

/* (slot, component, first unit) per 256 blocks of the window of every component a plane request wants.  Component 2 of a pair
 * (PLN_PAIRED) queues nothing: the lanes of component 1's items transform both. */
static void push_planes(std::vector<Work4> &L, uint32_t i, const DevPlanes &r)
{
	for (uint32_t c = 0; c < 4; ++c) {
		const DevPlane &p = r.c[c];
		if (!p.dst || (p.form == PLN_PAIRED && c == 2))
			continue;
		for (uint32_t f = 0, n = p.blk.w * p.blk.h; f < n; f += 256)
			L.push_back(Work4{i, c, f, 0u});
	}
}

/* (slot, component, first block) per 256 blocks of one component */
static void push_blocks(std::vector<Work4> &L, uint32_t i, const mij_image_desc &d, int comp)
{
	const uint32_t nblk = (uint32_t)(d.comp[comp].bw * d.comp[comp].bh);
	for (uint32_t f = 0; f < nblk; f += 256)
		L.push_back(Work4{i, (uint32_t)comp, f, 0u});
}

static void plan_decode(mij_batch *b, Plan &p)
{
	const size_t cap = (size_t)b->ctx->max_dyn_lds;
	for (Slot &s : b->slots) {
		s.choice = classify(b, s);
		if (s.reg)
			apply_region(s);
	}
	int auto_nb[MK_KINDS];
	auto_bands(b, auto_nb);
	for (size_t i = 0; i < b->slots.size(); ++i) {
		Slot &s = b->slots[i];
		const mij_image_desc &d = s.desc;
		const Choice &c = s.choice;
		s.work_items = 0;
		if (c.path == PATH_NONE)
			continue;
		if (host_staged(s) && s.coef_bytes_fmt && !(d.flags & MIJ_FLAG_STAGED_COMPACT)) /* int16 planes in the scratch -> compact planes */
			push_tiles(p.pack, (uint32_t)i, d);
		std::vector<Work4> &L = p.lists[c.kind][c.var];
		size_t &lds = p.lds[c.kind][c.var];
		const size_t before = L.size();
		switch (c.path) {
		case PATH_420:
		case PATH_440: /* band count by rounds of co-resident workgroups */
			if (s.reg) {
				push_region_bands(L, lds, (uint32_t)i, cap, c.path == PATH_420 ? LDS_COL_420 : LDS_COL_440, (int)s.win.y0, (int)(s.win.y0 + s.win.h), (int)s.win.x0,
										(int)(s.win.x0 + s.win.w), b->band_rows);
				break;
			}
			push_bands(L, lds, (uint32_t)i, d, c, b->band_rows > 0 ? (d.mcu_y + b->band_rows - 1) / b->band_rows : auto_nb[c.kind]);
			break;
		case PATH_422: { /* no halo: bands of about eight MCU rows keep the grid deep without making workgroups short */
			lds = c.lds > lds ? c.lds : lds;
			const int r0 = s.reg ? (int)s.win.y0 : 0, rows = s.reg ? (int)s.win.h : d.mcu_y; /* a region: its MCU rows, at full width */
			const int nb = (rows + 7) / 8;
			for (int k = 0; k < nb; ++k)
				L.push_back(Work4{(uint32_t)i, (uint32_t)(r0 + (long)rows * k / nb), (uint32_t)(r0 + (long)rows * (k + 1) / nb), 0u});
			break;
		}
		case PATH_GREY:
		case PATH_444:
		case PATH_1X1C:
			if (s.reg)
				push_window(L, (uint32_t)i, s.win);
			else
				push_blocks(L, (uint32_t)i, d, 0);
			break;
		case PATH_PLANES_OUT: /* (slot, component, first block of its window) per 256 blocks of every wanted component; a pair counts once */
			push_planes(L, (uint32_t)i, b->pln_req[(size_t)s.pln].dev);
			break;
		case PATH_SCALED: { /* 256 MCUs a workgroup; the luma-only form: 256 luma blocks */
			if (s.reg) {
				push_window(L, (uint32_t)i, s.win);
				break;
			}
			const uint32_t nm = c.kind == MK_SCALED + SC_Y ? (uint32_t)(d.comp[0].bw * d.comp[0].bh) : (uint32_t)(d.mcu_x * d.mcu_y);
			for (uint32_t f = 0; f < nm; f += 256)
				L.push_back(Work4{(uint32_t)i, 0u, f, 0u});
			break;
		}
		case PATH_LIBJPEG: { /* pass 2's items of MIJ_LJ_ITEM_W x MIJ_LJ_ITEM_H pixels in L, pass 1's blocks in the MK_LJ_IDCT list */
			for (uint32_t ty = 0; ty * MIJ_LJ_ITEM_H < (uint32_t)d.height; ++ty)
				for (uint32_t tx = 0; tx * MIJ_LJ_ITEM_W < (uint32_t)d.width; ++tx)
					L.push_back(Work4{(uint32_t)i, tx, ty, 0u});
			const int ncomp = c.kind == MK_LJ_COLOR + LJ_11 && (d.ncomp == 1 || d.n_out < 3) ? 1 : d.ncomp; /* luma alone: no chroma block is transformed */
			for (int comp = 0; comp < ncomp; ++comp)
				push_blocks(p.lists[MK_LJ_IDCT][s.coef_bytes_fmt ? 1 : 0], (uint32_t)i, d, comp);
			for (int comp = 0; comp < ncomp; ++comp) { /* its sample planes in the scratch arena, as the two-pass slots' */
				s.dev.comp[comp].plane_off = p.planes_need;
				p.planes_need += align_up((size_t)d.comp[comp].bw * 8 * d.comp[comp].bh * 8, 256);
			}
			break;
		}
		default: { /* PATH_TWO_PASS: pass 2's rows in L, pass 1's blocks in the MK_PLANES list */
			/* the vs == 2 forms of k_resample_fast take item r as output rows r-1 .. r+2 (row pairs around a chroma row) */
			const uint32_t r_end = (uint32_t)d.height + ((c.kind == MK_RS_FAST + RS_V2 || c.kind == MK_RS_FAST + RS_HV2) ? 2u : 0u);
			for (uint32_t r = 0; r < r_end; r += MIJ_RESAMPLE_ROWS)
				L.push_back(Work4{(uint32_t)i, 0u, r, 0u});
			const int wb = ((d.flags & MIJ_FLAG_WIDE_IDCT) ? 2 : 0) | (s.coef_bytes_fmt ? 1 : 0);
			for (int comp = 0; comp < d.ncomp; ++comp)
				push_blocks(p.lists[MK_PLANES][wb], (uint32_t)i, d, comp);
			/* rebase this image's sample planes into the scratch arena */
			for (int comp = 0; comp < d.ncomp; ++comp) {
				s.dev.comp[comp].plane_off = p.planes_need;
				p.planes_need += align_up((size_t)d.comp[comp].bw * 8 * d.comp[comp].bh * 8, 256);
			}
		}
		}
		s.work_items = (int)(L.size() - before);
		s.dev.src16_off = s.stage_off == MIJ_NO_STAGE ? 0 : s.stage_off;
	}
}

/* scratch planes for the two-pass path */
static int scratch_planes(mij_batch *b, size_t need)
{
	Grow grow(b->stream);
	grow.exact(b->planes, need);
	if (grow.hip != hipSuccess)
		return set_err(grow.hip == hipErrorOutOfMemory ? MIJ_E_NOMEM : MIJ_E_HIP, "scratch planes: %s", hipGetErrorString(grow.hip));
	return grow.rc;
}

/* Whether a launch takes k_fused420m where it would take k_fused420p: every picture of its list has rows of whole dwords (RGBA, or a width
 * that is a multiple of four), an output inside the 32-bit offsets of fused_band's fast strips (its `aligned`), and at most 2048 pixels a row,
 * two strips per lane -- and at least 16 MCU columns, below which a lane's second strip would be read from behind the workgroup's LDS
 * (mij_kernels.h, fused_band; MK_420 holds no picture that narrow as the forms are chosen now).  One picture that does not: the whole list stays. */
static bool band_march(const mij_batch *b, int kind, int var, size_t lds, const std::vector<Work4> &L)
{
	if (!MIJ_F420_MARCH || !band_prefetch(kind, var, lds, (size_t)b->ctx->max_dyn_lds) || !k420_march[var])
		return false;
	const uint32_t n_out = (var & 4) ? 4u : 3u;
	for (const Work4 &w : L) {
		const DevImage &d = b->slots[(size_t)w.a].dev;
		const bool dwords = n_out == 4 || (d.width & 3) == 0;
		const bool fits = (uint64_t)((uint32_t)d.width * n_out) * (uint32_t)d.height < 0xfffffff0ull;
		if (!dwords || !fits || d.width > 2048 || d.mcu_x < 16)
			return false;
	}
	return true;
}

/* work lists: the pack list first, then one range per launch in family and variant order; then the descriptors and the lists go up */
static int lay_out_work(mij_batch *b, const Plan &p)
{
	size_t total = p.pack.size();
	for (const auto &family : p.lists)
		for (const std::vector<Work4> &L : family)
			total += L.size();
	Grow grow(b->stream);
	grow(b->work, total);
	if (grow.rc != MIJ_OK)
		return grow.rc;
	b->launches.clear();
	if (!p.pack.empty())
		memcpy(b->work.h, p.pack.data(), p.pack.size() * sizeof(Work4));
	size_t pos = p.pack.size();
	for (int k = 0; k < MK_KINDS; ++k)
		for (int v = 0; v < MK_VARIANTS; ++v) {
			const std::vector<Work4> &L = p.lists[k][v];
			if (L.empty())
				continue;
			memcpy(b->work.h + pos, L.data(), L.size() * sizeof(Work4));
			b->launches.push_back(mij_batch::Launch{k, v, pos, L.size(), p.lds[k][v], band_march(b, k, v, p.lds[k][v], L)});
			pos += L.size();
		}
	const size_t n = b->slots.size();
	/* the row-extent tables as the band kernels read them: a byte per MCU row, two bits a component (the largest class of the component's
	 * block rows in that MCU row), each slot's at a multiple of eight bytes with eight bytes of room behind the last (the kernels read
	 * the aligned dword or two around a byte): a clone's is its source's, a rejected slot's is never read */
	size_t rc_bytes = 0;
	for (size_t i = 0; i < n; ++i) {
		b->slots[i].dev.rc_off = (uint32_t)rc_bytes;
		rc_bytes += align_up((size_t)b->slots[i].desc.mcu_y, 8);
	}
	rc_bytes += 8;
	if (rc_bytes > b->rc_room || rc_bytes > 0xffffffffull) /* cannot happen: see rc_room */
		return set_err(MIJ_E_NOMEM, "row-extent tables beyond their room in the coefficient arena");
	if (rc_bytes > b->rowcls.cap) {
		HIP_TRY(hipStreamSynchronize(b->stream)); /* an earlier upload's copy may still read the old one */
		HIP_TRY(b->rowcls.alloc(rc_bytes + rc_bytes / 2 + 64));
	}
	memset(b->rowcls.h, 0xff, rc_bytes);
	for (size_t i = 0; i < n; ++i) {
		const Slot &s = b->slots[i], &src = s.clone_of >= 0 ? b->slots[(size_t)s.clone_of] : s;
		uint8_t *row = b->rowcls.h + s.dev.rc_off;
		size_t at = 0;
		for (int c = 0; c < s.desc.ncomp && at + (size_t)s.desc.comp[c].bh <= src.rowcls.size(); at += (size_t)s.desc.comp[c].bh, ++c)
			for (int m = 0; m < s.desc.mcu_y; ++m) {
				uint8_t cls = 0;
				for (int v = 0; v < s.desc.comp[c].v; ++v)
					cls = std::max(cls, src.rowcls[at + (size_t)(m * s.desc.comp[c].v + v)]);
				row[m] = (uint8_t)((row[m] & ~(3u << (2 * c))) | ((unsigned)(cls & 3u) << (2 * c)));
			}
	}
	HIP_TRY(copy_table(b->coef.d, b->rowcls.h, rc_bytes, b->stream));
	for (size_t i = 0; i < n; ++i)
		b->imgs.h[i] = b->slots[i].dev;
	HIP_TRY(copy_table(b->imgs.d, b->imgs.h, sizeof(DevImage) * n, b->stream));
	bool windowed = false;
	for (const mij_batch::Launch &l : b->launches)
		windowed = windowed || families[l.kind].roi;
	if (windowed) { /* the windows of the slots the windowed kernels decode; the others' entries are never read */
		if (!b->roi.cap)
			HIP_TRY(b->roi.alloc((size_t)b->max_images));
		for (size_t i = 0; i < n; ++i)
			b->roi.h[i] = b->slots[i].reg ? b->slots[i].win : DevRoi{0u, 0u, 0u, 0u};
		HIP_TRY(copy_table(b->roi.d, b->roi.h, sizeof(DevRoi) * n, b->stream));
	}
	bool planes = false;
	for (const mij_batch::Launch &l : b->launches)
		planes = planes || families[l.kind].planes;
	if (planes) { /* the requests of the slots k_planes_out decodes; the others' entries are never read */
		if (!b->pln.cap)
			HIP_TRY(b->pln.alloc((size_t)b->max_images));
		for (const mij_batch::PlnReq &q : b->pln_req)
			b->pln.h[(size_t)q.slot] = q.dev;
		HIP_TRY(copy_table(b->pln.d, b->pln.h, sizeof(DevPlanes) * n, b->stream));
	}
	if (total)
		HIP_TRY(copy_table(b->work.d, b->work.h, sizeof(Work4) * total, b->stream));
	return MIJ_OK;
}

/* staged coefficients: own-staging slots are contiguous in the staging arena, the upload scratch and the coefficient arena in add
 * order, so runs of them with one destination go up in one copy each */
static int copy_coefficients(mij_batch *b)
{
	const size_t n = b->slots.size();
	size_t i = 0;
	while (i < n) {
		if (!host_staged(b->slots[i]) || (b->slots[i].desc.flags & MIJ_FLAG_SKIP)) {
			++i;
			continue;
		}
		if (b->slots[i].desc.flags & MIJ_FLAG_STAGED_COMPACT) { /* compact planes written by the host stage: straight to their place, escape region only when used */
			const Slot &sc = b->slots[i];
			/* small pictures: a run of neighbours goes up in ONE copy, escape regions and all (unused ones carry whatever the staging arena held:
			 * nothing reads them) -- a batch of 8192 thumbnails paid 8192 copy calls, 40 ms, where the int16 staging of round 2 went up in one */
			const size_t small = (size_t)1 << 20;
			if (sc.coef_bytes <= small) {
				size_t j = i, bytes = 0;
				while (j < n && host_staged(b->slots[j]) && !(b->slots[j].desc.flags & MIJ_FLAG_SKIP) && (b->slots[j].desc.flags & MIJ_FLAG_STAGED_COMPACT) &&
						 b->slots[j].coef_bytes <= small && b->slots[j].stage_off == sc.stage_off + bytes && b->slots[j].coef_base == sc.coef_base + bytes) {
					bytes += b->slots[j].coef_bytes;
					++j;
				}
				HIP_TRY(hipMemcpyAsync(b->coef.d + sc.coef_base, b->stage.h + sc.stage_off, bytes, hipMemcpyHostToDevice, b->stream));
				i = j;
				continue;
			}
			const size_t main_bytes = mij_compact_main_bytes(&sc.desc);
			HIP_TRY(hipMemcpyAsync(b->coef.d + sc.coef_base, b->stage.h + sc.stage_off, (sc.desc.flags & MIJ_FLAG_HAS_ESCAPES) ? sc.coef_bytes : main_bytes, hipMemcpyHostToDevice, b->stream));
			++i;
			continue;
		}
		size_t j = i, bytes = 0;
		const int fmt = b->slots[i].coef_bytes_fmt;
		const size_t s0 = b->slots[i].stage_off, c0 = b->slots[i].coef_base;
		while (j < n && host_staged(b->slots[j]) && !(b->slots[j].desc.flags & (MIJ_FLAG_SKIP | MIJ_FLAG_STAGED_COMPACT)) && b->slots[j].coef_bytes_fmt == fmt &&
				 b->slots[j].stage_off == s0 + bytes && b->slots[j].coef_base == c0 + bytes) {
			bytes += b->slots[j].coef_bytes;
			++j;
		}
		HIP_TRY(hipMemcpyAsync(fmt ? b->up16.d + s0 : b->coef.d + c0, b->stage.h + s0, bytes, hipMemcpyHostToDevice, b->stream));
		i = j;
	}
	return MIJ_OK;
}

/* k_pack_c8 over the pack list (the head of the work list), between the events mij_batch_pack_ms reads */
static int launch_pack(mij_batch *b, size_t items)
{
	b->pack_timed = false;
	if (!items)
		return MIJ_OK;
	if (!b->ev_pack0) {
		HIP_TRY(hipEventCreate(&b->ev_pack0));
		HIP_TRY(hipEventCreate(&b->ev_pack1));
	}
	HIP_TRY(hipEventRecord(b->ev_pack0, b->stream));
	hipLaunchKernelGGL(k_pack_c8, dim3((unsigned)items), dim3(256), 0, b->stream, b->imgs.d, reinterpret_cast<const WorkIdct *>(b->work.d), b->up16.d, b->coef.d, b->l1max.d);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(b->ev_pack1, b->stream));
	b->pack_timed = true;
	return MIJ_OK;
}

/* clones: their source's planes, device to device */
static int copy_clones(mij_batch *b)
{
	for (const Slot &s : b->slots)
		if (s.clone_of >= 0)
			HIP_TRY(hipMemcpyAsync(b->coef.d + s.coef_base, b->coef.d + b->slots[(size_t)s.clone_of].coef_base, s.coef_bytes, hipMemcpyDeviceToDevice, b->stream));
	return MIJ_OK;
}

extern "C" int mij_batch_upload(mij_batch *b)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	HIP_TRY(hipSetDevice(b->ctx->device));
	if (b->slots.empty())
		return set_err(MIJ_E_STATE, "batch is empty");
	for (size_t i = 0; i < b->slots.size(); ++i) /* flags and colour may have changed since mij_batch_set_scale */
		if (b->slots[i].scale > 1 && !(b->slots[i].desc.flags & MIJ_FLAG_SKIP) && scaled_layout(b->slots[i].desc) < 0)
			return set_err(MIJ_E_ARG, "mij_batch_upload: slot %zu cannot be decoded at 1/%d size", i, b->slots[i].scale);
	for (size_t i = 0; i < b->slots.size(); ++i) /* ... and since mij_batch_set_arith */
		if (b->slots[i].arith == MIJ_ARITH_LIBJPEG && !(b->slots[i].desc.flags & MIJ_FLAG_SKIP) && lj_layout(b->slots[i].desc) < 0)
			return set_err(MIJ_E_ARG, "mij_batch_upload: slot %zu cannot be decoded with libjpeg's arithmetic", i);
	Plan p;
	int rc;
	if ((rc = resolve_regions(b)) != MIJ_OK)
		return rc;
	if ((rc = plane_formats(b)) != MIJ_OK || (rc = l1_prepack(b)) != MIJ_OK)
		return rc;
	plan_decode(b, p);
	if ((rc = scratch_planes(b, p.planes_need)) != MIJ_OK || (rc = lay_out_work(b, p)) != MIJ_OK || (rc = copy_coefficients(b)) != MIJ_OK ||
		 (rc = launch_pack(b, p.pack.size())) != MIJ_OK || (rc = copy_clones(b)) != MIJ_OK)
		return rc;
	if ((rc = f32_plan(b)) != MIJ_OK || (rc = ten_plan(b, false)) != MIJ_OK || (rc = rsz_plan(b, false)) != MIJ_OK || (rc = ten_plan(b, true)) != MIJ_OK ||
		 (rc = rsz_plan(b, true)) != MIJ_OK)
		return rc;
	b->uploaded = true;
	b->launched = false;
	return MIJ_OK;
}

/* One output pass on the batch stream, if its plan has work items: a kernel that takes the plan's descriptors, work list and tables, then
 * `tail`.  A batch without such requests launches nothing. */
template <typename Dev, typename Work, typename Lut, typename... Params, typename... Args>
static int launch_out_pass(mij_batch *b, const PlanBuf &p, void (*kernel)(const Dev *, const Work *, const Lut *, Params...), Args... tail)
{
	if (!p.items)
		return MIJ_OK;
	hipLaunchKernelGGL(kernel, dim3((unsigned)p.items), dim3(256), 0, b->stream, reinterpret_cast<const Dev *>(p.buf.d), reinterpret_cast<const Work *>(p.buf.d + p.work_at),
							 reinterpret_cast<const Lut *>(p.buf.d + p.lut_at), tail...);
	HIP_TRY(hipGetLastError());
	return MIJ_OK;
}

extern "C" int mij_batch_launch(mij_batch *b)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	if (!b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_launch before mij_batch_upload");
	HIP_TRY(hipSetDevice(b->ctx->device));
	for (const auto &L : b->launches) { /* in family order: pass 2 of the two-pass family runs behind every pass-1 launch */
		const Family &f = families[L.kind];
		const Work4 *wk = b->work.d + L.first;
		const uint8_t *in = f.io == PLANES_OUT ? b->planes.d : b->coef.d;
		uint8_t *out = f.io == COEF_PLANES ? b->planes.d : b->out.d;
		/* the windowed forms take the table of windows, k_planes_out the table of plane requests */
		void *args4[] = {&b->imgs.d, &wk, &in, &out}, *args5[] = {&b->imgs.d, &wk, &in, &out, f.planes ? (void *)&b->pln.d : (void *)&b->roi.d};
		const void *k = L.marched ? k420_march[L.var] : (band_prefetch(L.kind, L.var, L.lds, (size_t)b->ctx->max_dyn_lds) ? k420_prefetch[L.var] : f.k[L.var]);
		(void)hipLaunchKernel(k, dim3((unsigned)L.count), dim3(f.threads), (f.roi || f.planes) ? args5 : args4, L.lds, b->stream);
		HIP_TRY(hipGetLastError());
	}
	/* the output passes, behind every decode family (both front ends end here): float output, tensor output into the callers' memory,
	 * resized tensor output, then the transposed (oriented 5..8) forms of the last two */
	int rc;
	if ((rc = launch_out_pass(b, b->f32plan, k_out_f32, b->out.d, b->f32.d)) != MIJ_OK || (rc = launch_out_pass(b, b->tenplan, k_out_tensor, b->out.d)) != MIJ_OK ||
		 (rc = launch_out_pass(b, b->rszplan, k_out_resize, b->rszplan.buf.d, b->out.d)) != MIJ_OK ||
		 (rc = launch_out_pass(b, b->tentplan, k_out_tensor_t, b->out.d)) != MIJ_OK ||
		 (rc = launch_out_pass(b, b->rsztplan, k_out_resize_t, b->rsztplan.buf.d, b->out.d)) != MIJ_OK)
		return rc;
	b->launched = true;
	return MIJ_OK;
}

extern "C" int mij_batch_submit(mij_batch *b)
{
	int rc = mij_batch_upload(b);
	if (rc != MIJ_OK)
		return rc;
	return mij_batch_launch(b);
}

extern "C" int mij_batch_wait(mij_batch *b)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	HIP_TRY(hipSetDevice(b->ctx->device));
	HIP_TRY(hipStreamSynchronize(b->stream));
	return MIJ_OK;
}

extern "C" int mij_batch_fetch(mij_batch *b, int slot, uint8_t *dst, size_t dst_bytes)
{
	if (!dst || !batch_slot(b, slot))
		return set_err(MIJ_E_ARG, "bad slot or destination");
	if (!b->launched)
		return set_err(MIJ_E_STATE, "mij_batch_fetch before launch");
	const Slot &s = b->slots[(size_t)slot];
	if (s.desc.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_STATE, "slot %d was rejected by the host stage", slot);
	if (s.pln >= 0)
		return set_err(MIJ_E_STATE, "mij_batch_fetch: slot %d has a plane request: it decodes no pixels", slot);
	const size_t bytes = out_px_bytes(s);
	if (dst_bytes < bytes)
		return set_err(MIJ_E_ARG, "destination too small (%zu < %zu)", dst_bytes, bytes);
	HIP_TRY(hipSetDevice(b->ctx->device));
	return d2h_bounced(b->ctx, b->stream, dst, b->out.d + s.dev.out_off, bytes);
}

extern "C" int mij_batch_fetch_all_async(mij_batch *b, uint8_t *dst, size_t dst_bytes)
{
	if (!b || !dst)
		return set_err(MIJ_E_ARG, "bad batch or destination");
	if (!b->launched)
		return set_err(MIJ_E_STATE, "mij_batch_fetch_all_async before launch");
	if (dst_bytes < b->out_used)
		return set_err(MIJ_E_ARG, "destination too small (%zu < %zu)", dst_bytes, b->out_used);
	HIP_TRY(hipSetDevice(b->ctx->device));
	if (b->out_used)
		HIP_TRY(hipMemcpyAsync(dst, b->out.d, b->out_used, hipMemcpyDeviceToHost, b->stream));
	return MIJ_OK;
}

extern "C" size_t mij_batch_out_offset(const mij_batch *b, int slot)
{
	if (!batch_slot(b, slot))
		return (size_t)-1;
	return (size_t)b->slots[(size_t)slot].dev.out_off;
}

extern "C" size_t mij_batch_out_bytes(const mij_batch *b) { return b ? b->out_used : 0; }

extern "C" void *mij_host_alloc(size_t bytes)
{
	void *p = nullptr;
	if (hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess) {
		(void)hipGetLastError();
		set_err(MIJ_E_NOMEM, "pinned host allocation of %zu bytes failed", bytes);
		return nullptr;
	}
	return p;
}

extern "C" void mij_host_free(void *p)
{
	if (p)
		(void)hipHostFree(p);
}

extern "C" void *mij_batch_device_out(mij_batch *b, int slot)
{
	if (!batch_slot(b, slot))
		return nullptr;
	return b->out.d + b->slots[(size_t)slot].dev.out_off;
}

/* ------------------------------------------------------------------ float output */

extern "C" size_t mij_image_out_f32_bytes(const mij_image_desc *d) { return align_up(4 * (size_t)d->n_out * d->width * d->height, 256); }

extern "C" int mij_batch_out_f32_reserve(mij_batch *b, size_t bytes)
{
	if (!b || !bytes)
		return set_err(MIJ_E_ARG, "mij_batch_out_f32_reserve: bad argument");
	if (bytes <= b->f32.cap)
		return MIJ_OK;
	if (!b->f32_req.empty())
		return set_err(MIJ_E_STATE, "mij_batch_out_f32_reserve: slots hold float requests (reset the batch first)");
	HIP_TRY(hipSetDevice(b->ctx->device));
	HIP_TRY(hipStreamSynchronize(b->stream));
	/* the new arena first, so that a failure leaves the old one in place; only when memory is short does the old one go first */
	const size_t cap = align_up(bytes, 256);
	Buf<uint8_t, BUF_ON_DEVICE> arena;
	hipError_t e = arena.alloc(cap);
	if (e == hipErrorOutOfMemory && b->f32.d) {
		(void)hipGetLastError();
		b->f32.release();
		e = arena.alloc(cap);
	}
	if (e != hipSuccess) {
		(void)hipGetLastError();
		return set_err(e == hipErrorOutOfMemory ? MIJ_E_NOMEM : MIJ_E_HIP, "mij_batch_out_f32_reserve: %s", hipGetErrorString(e));
	}
	b->f32 = std::move(arena); /* arena takes the old one and releases it */
	return MIJ_OK;
}

extern "C" int mij_batch_set_out_f32(mij_batch *b, int slot, const float *lut)
{
	if (!lut || !batch_slot(b, slot))
		return set_err(MIJ_E_ARG, "mij_batch_set_out_f32: bad slot or table");
	if (b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_set_out_f32 after mij_batch_upload");
	Slot &s = b->slots[(size_t)slot];
	if (s.desc.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_STATE, "slot %d was rejected by the host stage", slot);
	if (s.pln >= 0)
		return set_err(MIJ_E_STATE, "mij_batch_set_out_f32: slot %d has a plane request: it decodes no pixels", slot);
	if (s.scale > 1)
		return set_err(MIJ_E_ARG, "mij_batch_set_out_f32: slot %d is decoded at 1/%d size; float output of reduced pictures is not supported", slot, s.scale);
	if (wants_region(s))
		return set_err(MIJ_E_ARG, "mij_batch_set_out_f32: slot %d decodes a region only; float output of a region is not supported", slot);
	if (s.f32 < 0) {
		const size_t need = mij_image_out_f32_bytes(&s.desc);
		if (!b->f32.d || b->f32_used + need > b->f32.cap)
			return set_err(MIJ_E_ARG, "float arena too small (%zu of %zu bytes used, %zu needed; mij_batch_out_f32_reserve)", b->f32_used, b->f32.cap, need);
		mij_batch::F32Req q;
		q.slot = slot;
		q.off = b->f32_used;
		b->f32_req.push_back(q);
		b->f32_used += need;
		s.f32 = (int)b->f32_req.size() - 1;
	}
	float *t = b->f32_req[(size_t)s.f32].lut;
	memset(t, 0, sizeof(float) * MIJ_F32_LUT_FLOATS);
	memcpy(t, lut, sizeof(float) * 256 * (size_t)s.desc.n_out);
	return MIJ_OK;
}

extern "C" int mij_batch_fetch_f32(mij_batch *b, int slot, float *dst, size_t dst_elems)
{
	if (!dst || !batch_slot(b, slot))
		return set_err(MIJ_E_ARG, "bad slot or destination");
	const Slot &s = b->slots[(size_t)slot];
	if (s.f32 < 0)
		return set_err(MIJ_E_STATE, "slot %d has no float output (mij_batch_set_out_f32)", slot);
	if (!b->launched)
		return set_err(MIJ_E_STATE, "mij_batch_fetch_f32 before launch");
	if (s.desc.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_STATE, "slot %d was rejected by the host stage", slot);
	const size_t elems = (size_t)s.desc.n_out * s.desc.width * s.desc.height;
	if (dst_elems < elems)
		return set_err(MIJ_E_ARG, "destination too small (%zu < %zu floats)", dst_elems, elems);
	HIP_TRY(hipSetDevice(b->ctx->device));
	return d2h_bounced(b->ctx, b->stream, dst, b->f32.d + b->f32_req[(size_t)s.f32].off, elems * sizeof(float));
}

extern "C" void *mij_batch_device_out_f32(mij_batch *b, int slot)
{
	const Slot *s = batch_slot(b, slot);
	if (!s || s->f32 < 0)
		return nullptr;
	return b->f32.d + b->f32_req[(size_t)s->f32].off;
}

/* ------------------------------------------------------------------ tensor output */

/* One axis of a resized request: the coefficients of mjh_resize_coeffs, cached per (in, out, filter) until reset, and checked against
 * the kernel's arithmetic.  An axis whose size does not change gets the identity (one tap of 2^22 per output), which gives back the
 * input bytes exactly: the contract skips that pass. */
static const mij_batch::RszCoef *rsz_coef(mij_batch *b, int in, int out, int filter, bool mirror = false)
{
	const uint64_t key = ((uint64_t)(uint32_t)in << 32) | ((uint64_t)(uint32_t)out << 3) | (uint64_t)(uint32_t)(in == out ? 7 : filter) |
								(mirror && in != out ? (uint64_t)1 << 24 : 0);
	auto it = b->rsz_coef.find(key);
	if (it != b->rsz_coef.end())
		return &it->second;
	mij_batch::RszCoef c;
	if (mirror && in != out) {
		/* the axis read backwards: output o of the mirrored input is output out-1-o of the input, mirrored.  lo* = in - lo - n of
		 * out-1-o, its taps reversed, stays ascending; the request's flip of the axis is toggled (set_out_tensor). */
		const mij_batch::RszCoef *f = rsz_coef(b, in, out, filter, false);
		if (!f)
			return nullptr;
		c = *f;
		const size_t ks = (size_t)c.ks;
		for (int o = 0; o < out; ++o) {
			const size_t m = (size_t)(out - 1 - o);
			const int32_t lo = f->v[2 * m], n = f->v[2 * m + 1];
			c.v[2 * (size_t)o] = in - lo - n;
			c.v[2 * (size_t)o + 1] = n;
			int32_t *k = c.v.data() + 2 * (size_t)out + (size_t)o * ks;
			const int32_t *fk = f->v.data() + 2 * (size_t)out + m * ks;
			for (int t = 0; t < n; ++t)
				k[t] = fk[n - 1 - t];
		}
		return &b->rsz_coef.emplace(key, std::move(c)).first->second;
	}
	if (in == out) {
		c.ks = 1;
		c.v.resize((size_t)out * 3);
		for (int o = 0; o < out; ++o) {
			c.v[2 * (size_t)o] = o;
			c.v[2 * (size_t)o + 1] = 1;
			c.v[2 * (size_t)out + o] = 1 << 22;
		}
	} else {
		c.ks = mjh_resize_coeffs(in, out, filter, nullptr, nullptr, 0);
		if (c.ks < 1)
			return nullptr;
		c.v.resize((size_t)out * (2 + (size_t)c.ks));
		if (mjh_resize_coeffs(in, out, filter, c.v.data(), c.v.data() + 2 * (size_t)out, (size_t)out * c.ks) != c.ks)
			return nullptr;
	}
	/* 24-bit multiplies take |k| < 2^23; a 32-bit sum of 2^21 and n products of a byte cannot overflow while 255 * sum |k| < 2^31 - 2^21 */
	c.big = false;
	c.fits = true;
	for (int o = 0; o < out; ++o) {
		int64_t sum = 0;
		const int32_t *k = c.v.data() + 2 * (size_t)out + (size_t)o * c.ks;
		for (int t = 0; t < c.ks; ++t) {
			const int64_t a = k[t] < 0 ? -(int64_t)k[t] : k[t];
			sum += a;
			c.big |= a >= ((int64_t)1 << 23);
		}
		c.fits &= 255 * sum < ((int64_t)1 << 31) - ((int64_t)1 << 21);
	}
	return &b->rsz_coef.emplace(key, std::move(c)).first->second;
}

/* MIJ_OK when the `extent` bytes from p are device memory of `device`, inside the one allocation hipMemGetAddressRange reports for p
 * (a range that cannot be determined is refused too); else MIJ_E_ARG naming p as `what` */
static int device_extent(int device, const void *p, uint64_t extent, const char *what)
{
	HIP_TRY(hipSetDevice(device));
	hipPointerAttribute_t pa;
	memset(&pa, 0, sizeof(pa));
	hipError_t e = hipPointerGetAttributes(&pa, p);
	if (e != hipSuccess || pa.type != hipMemoryTypeDevice || pa.isManaged || pa.device != device) {
		(void)hipGetLastError();
		return set_err(MIJ_E_ARG, "%s %p is not device memory of device %d", what, p, device);
	}
	hipDeviceptr_t base = nullptr;
	size_t size = 0;
	const uintptr_t a = (uintptr_t)p;
	e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p);
	if (e != hipSuccess || !base || a < (uintptr_t)base || a - (uintptr_t)base > size || extent > size - (a - (uintptr_t)base)) {
		(void)hipGetLastError();
		return set_err(MIJ_E_ARG, "the %llu bytes from %s %p are not inside one allocation (%p, %zu bytes)", (unsigned long long)extent, what, p, (void *)base,
							size);
	}
	return MIJ_OK;
}

/* o = 1..8 as (transpose, mirror the stored x axis, mirror the stored y axis): D is (S mirrored)^T when transposed (include/mij.h) */
static const uint8_t orient_tr[9] = {0, 0, 0, 0, 0, 1, 1, 1, 1}, orient_mx[9] = {0, 0, 1, 1, 0, 0, 0, 1, 1}, orient_my[9] = {0, 0, 0, 1, 1, 0, 1, 1, 0};

static int set_out_tensor(mij_batch *b, int slot, const mij_out_tensor *t, const mij_out_resize *rz, int32_t orient, const void *table)
{
	if (!t || !batch_slot(b, slot))
		return set_err(MIJ_E_ARG, "mij_batch_set_out_tensor: bad slot or request");
	if (b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_set_out_tensor after mij_batch_upload");
	Slot &s = b->slots[(size_t)slot];
	if (s.desc.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_STATE, "slot %d was rejected by the host stage", slot);
	if (s.pln >= 0)
		return set_err(MIJ_E_STATE, "mij_batch_set_out_tensor: slot %d has a plane request: it decodes no pixels", slot);
	if (t->dtype < MIJ_DT_U8 || t->dtype > MIJ_DT_F32 || (t->layout != MIJ_LAYOUT_HWC && t->layout != MIJ_LAYOUT_CHW))
		return set_err(MIJ_E_ARG, "mij_batch_set_out_tensor: dtype %d / layout %d unknown", t->dtype, t->layout);
	if (!table && t->dtype != MIJ_DT_U8)
		return set_err(MIJ_E_ARG, "mij_batch_set_out_tensor: a table is required for dtype %d", t->dtype);
	if (orient < 1 || orient > 8)
		return set_err(MIJ_E_ARG, "mij_batch_set_out_tensor_oriented: orientation %d is not 1..8", (int)orient);
	const bool tr = orient_tr[orient], mx = orient_mx[orient], my = orient_my[orient];
	const int64_t W = out_w(s), H = out_h(s), C = s.desc.n_out; /* the stored picture: reduced when the slot has a scale */
	const int64_t DW = tr ? H : W, DH = tr ? W : H; /* the displayed picture */
	if (t->w < 1 || t->h < 1 || t->x0 < 0 || t->y0 < 0 || (int64_t)t->x0 + t->w > DW || (int64_t)t->y0 + t->h > DH)
		return set_err(MIJ_E_ARG, "window %d,%d %dx%d outside the %lldx%lld displayed picture of slot %d (orientation %d)", t->x0, t->y0, t->w, t->h,
							(long long)DW, (long long)DH, slot, (int)orient);
	/* the axes of the window: D's x axis is S's y axis when transposed; an axis S reads backwards is mirrored */
	const bool mirror_x = tr ? my : mx, mirror_y = tr ? mx : my;
	const mij_batch::RszCoef *ch = nullptr, *cv = nullptr;
	if (rz) {
		if (rz->filter < MIJ_FILTER_BOX || rz->filter > MIJ_FILTER_LANCZOS || rz->reserved != 0 || rz->out_w < 1 || rz->out_w > 16384 || rz->out_h < 1 ||
			 rz->out_h > 16384)
			return set_err(MIJ_E_ARG, "mij_batch_set_out_tensor_resized: %dx%d filter %d reserved %d refused", rz->out_w, rz->out_h, rz->filter, rz->reserved);
		ch = rsz_coef(b, t->w, rz->out_w, rz->filter, mirror_x);
		cv = rsz_coef(b, t->h, rz->out_h, rz->filter, mirror_y);
		if (!ch || !cv)
			return set_err(MIJ_E_ARG, "mij_batch_set_out_tensor_resized: no coefficients for %dx%d -> %dx%d", t->w, t->h, rz->out_w, rz->out_h);
		if (!ch->fits || !cv->fits)
			return set_err(MIJ_E_ARG, "mij_batch_set_out_tensor_resized: %dx%d -> %dx%d filter %d: coefficients could overflow 32-bit sums", t->w, t->h,
								rz->out_w, rz->out_h, rz->filter);
	}
	const bool chw = t->layout == MIJ_LAYOUT_CHW;
	/* the extent written: the window, or the resized window */
	const int64_t w = rz ? rz->out_w : t->w, h = rz ? rz->out_h : t->h, rp = t->row_pitch, pp = chw ? t->plane_pitch : 0;
	const int64_t lim = (int64_t)1 << 40; /* keeps the extent below in range */
	if (rp < 0 || rp > lim || pp < 0 || pp > lim)
		return set_err(MIJ_E_ARG, "pitch out of range (row %lld, plane %lld)", (long long)rp, (long long)pp);
	const int64_t line = chw ? w : w * C;
	if ((h > 1 && rp < line) || (chw && C > 1 && pp < (h - 1) * rp + w))
		return set_err(MIJ_E_ARG, "pitches let rows or planes overlap (row %lld, plane %lld; %lldx%lldx%lld %s)", (long long)rp, (long long)pp, (long long)w,
							(long long)h, (long long)C, chw ? "CHW" : "HWC");
	const uint32_t es = t->dtype == MIJ_DT_U8 ? 1u : (t->dtype == MIJ_DT_F32 ? 4u : 2u);
	const uintptr_t dst = (uintptr_t)t->dst;
	if (!dst || (dst & (es - 1u)))
		return set_err(MIJ_E_ARG, "dst %p is not aligned to its %u-byte elements", t->dst, es);
	const uint64_t last = (uint64_t)((h - 1) * rp + (chw ? (C - 1) * pp + w - 1 : w * C - 1)); /* element offset of the last element */
	const uint64_t extent = (last + 1) * es;
	const int rc = device_extent(b->ctx->device, t->dst, extent, "dst");
	if (rc != MIJ_OK)
		return rc;
	if (s.ten < 0) {
		b->ten_req.emplace_back();
		b->ten_req.back().slot = slot;
		s.ten = (int)b->ten_req.size() - 1;
	}
	mij_batch::TenReq &q = b->ten_req[(size_t)s.ten];
	q.t = *t;
	/* into the stored frame: the window's corner in S, and each mirror composed with the flip of its output axis (for a resize, with
	 * that axis's coefficients mirrored above: resize(mirror(x)) = mirror(resize*(x)) exactly) */
	q.tr = tr;
	if (tr) {
		q.t.x0 = mx ? (int32_t)(W - t->y0 - t->h) : t->y0; /* output rows are stored columns */
		q.t.y0 = my ? (int32_t)(H - t->x0 - t->w) : t->x0; /* output columns are stored rows */
	} else {
		q.t.x0 = mx ? (int32_t)(W - t->x0 - t->w) : t->x0;
		q.t.y0 = my ? (int32_t)(H - t->y0 - t->h) : t->y0;
	}
	q.t.flip_x = (t->flip_x ? 1 : 0) ^ (mirror_x ? 1 : 0);
	q.t.flip_y = (t->flip_y ? 1 : 0) ^ (mirror_y ? 1 : 0);
	q.rsz = rz != nullptr;
	if (rz) {
		q.r = *rz;
		q.ch = ch;
		q.cv = cv;
	}
	q.esize = es;
	q.lut = table != nullptr;
	memset(q.table, 0, sizeof(q.table));
	if (table)
		memcpy(q.table, table, (size_t)es * 256 * (size_t)C);
	return MIJ_OK;
}

extern "C" int mij_batch_set_out_tensor(mij_batch *b, int slot, const mij_out_tensor *t, const void *table)
{
	return set_out_tensor(b, slot, t, nullptr, 1, table);
}

extern "C" int mij_batch_set_out_tensor_resized(mij_batch *b, int slot, const mij_out_tensor *t, const mij_out_resize *r, const void *table)
{
	if (!r)
		return set_err(MIJ_E_ARG, "mij_batch_set_out_tensor_resized: no resize");
	return set_out_tensor(b, slot, t, r, 1, table);
}

extern "C" int mij_batch_set_out_tensor_oriented(mij_batch *b, int slot, const mij_out_tensor *t, const mij_out_resize *r, int32_t orientation,
																 const void *table)
{
	return set_out_tensor(b, slot, t, r, orientation, table);
}

/* ------------------------------------------------------------------ plane output (include/mij.h, PLANE OUTPUT) */

static inline uint32_t low_bit(uint64_t v, uint32_t cap)
{
	uint32_t a = 1;
	while (a < cap && !(v & a))
		a <<= 1;
	return a;
}

extern "C" int mij_batch_set_out_planes(mij_batch *b, int slot, const mij_out_planes *p)
{
	if (!p || !batch_slot(b, slot))
		return set_err(MIJ_E_ARG, "mij_batch_set_out_planes: bad slot or request");
	if (b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_set_out_planes after mij_batch_upload");
	Slot &s = b->slots[(size_t)slot];
	const mij_image_desc &d = s.desc;
	if (d.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_STATE, "slot %d was rejected by the host stage", slot);
	if (s.f32 >= 0 || s.ten >= 0)
		return set_err(MIJ_E_STATE, "mij_batch_set_out_planes: slot %d already has a %s request; a slot holds one kind", slot, s.f32 >= 0 ? "float" : "tensor");
	if (s.scale > 1 || wants_region(s))
		return set_err(MIJ_E_STATE, "mij_batch_set_out_planes: slot %d has a %s; planes are decoded at full size through the request's own window", slot,
							s.scale > 1 ? "scale" : "region");
	if (s.arith == MIJ_ARITH_LIBJPEG)
		return set_err(MIJ_E_STATE, "mij_batch_set_out_planes: slot %d is decoded with libjpeg's arithmetic; plane output has the reference's samples only", slot);
	if (p->reserved[0] || p->reserved[1])
		return set_err(MIJ_E_ARG, "mij_batch_set_out_planes: reserved is not 0");
	int64_t x0 = p->x0, y0 = p->y0, w = p->w, h = p->h;
	if (!x0 && !y0 && !w && !h)
		w = d.width, h = d.height;
	if (w < 1 || h < 1 || x0 < 0 || y0 < 0 || x0 + w > d.width || y0 + h > d.height)
		return set_err(MIJ_E_ARG, "mij_batch_set_out_planes: window %d,%d %dx%d is empty or outside the %dx%d picture of slot %d", p->x0, p->y0, p->w, p->h, d.width,
							d.height, slot);
	mij_batch::PlnReq q;
	q.slot = slot;
	memset(&q.dev, 0, sizeof(q.dev));
	int wanted = 0;
	const int64_t lim = (int64_t)1 << 40; /* keeps the extent below in range */
	for (int c = 0; c < 4; ++c) {
		const mij_out_plane &pl = p->planes[c];
		if (!pl.dst)
			continue;
		if (c >= d.ncomp)
			return set_err(MIJ_E_ARG, "mij_batch_set_out_planes: a plane for component %d, slot %d has %d", c, slot, d.ncomp);
		const mij_comp_desc &cp = d.comp[c];
		if ((x0 * cp.h) % d.h_max || (y0 * cp.v) % d.v_max)
			return set_err(MIJ_E_ARG, "mij_batch_set_out_planes: window origin %d,%d is off the grid of component %d (%dx%d of %dx%d)", p->x0, p->y0, c, cp.h, cp.v,
								d.h_max, d.v_max);
		const int64_t sx0 = x0 * cp.h / d.h_max, sy0 = y0 * cp.v / d.v_max;
		const int64_t sx1 = std::min<int64_t>(((x0 + w) * cp.h + d.h_max - 1) / d.h_max, cp.x), sy1 = std::min<int64_t>(((y0 + h) * cp.v + d.v_max - 1) / d.v_max, cp.y);
		if (sx1 <= sx0 || sy1 <= sy0)
			return set_err(MIJ_E_ARG, "mij_batch_set_out_planes: the window holds no sample of component %d", c);
		const int64_t wc = sx1 - sx0, hc = sy1 - sy0, rp = pl.row_pitch, xp = pl.x_pitch;
		if (rp < 1 || xp < 1 || rp > lim || xp > lim)
			return set_err(MIJ_E_ARG, "mij_batch_set_out_planes: component %d: pitches %lld, %lld are not positive (or beyond 2^40)", c, (long long)rp, (long long)xp);
		if (hc > 1 && rp < (wc - 1) * xp + 1)
			return set_err(MIJ_E_ARG, "mij_batch_set_out_planes: component %d: row pitch %lld lets its rows of %lld samples %lld bytes apart overlap", c, (long long)rp,
								(long long)wc, (long long)xp);
		const uint64_t extent = (uint64_t)((hc - 1) * rp + (wc - 1) * xp + 1);
		const int rc = device_extent(b->ctx->device, pl.dst, extent, "plane dst");
		if (rc != MIJ_OK)
			return rc;
		DevPlane &v = q.dev.c[c];
		v.dst = (uint64_t)(uintptr_t)pl.dst;
		v.row_pitch = rp;
		v.x_pitch = xp;
		v.sx0 = (uint32_t)sx0, v.sy0 = (uint32_t)sy0, v.sx1 = (uint32_t)sx1, v.sy1 = (uint32_t)sy1;
		v.blk = DevRoi{(uint32_t)(sx0 >> 3), (uint32_t)(sy0 >> 3), (uint32_t)(((sx1 + 7) >> 3) - (sx0 >> 3)), (uint32_t)(((sy1 + 7) >> 3) - (sy0 >> 3))};
		/* fast form: every block's row starts 8-byte aligned (dst + (8 by - sy0) * rp + 8 bx - sx0) */
		v.form = (xp == 1 && !((v.dst - (uint64_t)sx0) & 7u) && !(rp & 7)) ? PLN_FAST : PLN_GENERAL;
		++wanted;
	}
	if (!wanted)
		return set_err(MIJ_E_ARG, "mij_batch_set_out_planes: no component is wanted");
	/* paired form (NV12 / NV21): components 1 and 2 of one geometry and rectangle, two bytes a sample, one byte apart, on an even base */
	DevPlane &u = q.dev.c[1], &v = q.dev.c[2];
	if (u.dst && v.dst && u.x_pitch == 2 && v.x_pitch == 2 && u.row_pitch == v.row_pitch && d.comp[1].bw == d.comp[2].bw && d.comp[1].bh == d.comp[2].bh &&
		 u.sx0 == v.sx0 && u.sy0 == v.sy0 && u.sx1 == v.sx1 && u.sy1 == v.sy1 && (u.dst + 1 == v.dst || v.dst + 1 == u.dst)) {
		const uint64_t base = std::min(u.dst, v.dst);
		const uint32_t align = low_bit((base - 2u * (uint64_t)u.sx0) | (uint64_t)u.row_pitch, 16u);
		if (align >= 2u) {
			const uint32_t first = u.dst < v.dst ? 1u : 2u;
			u.form = v.form = PLN_PAIRED;
			u.dst = v.dst = base;
			u.first = v.first = first;
			u.align = v.align = align;
		}
	}
	if (s.pln < 0) {
		b->pln_req.push_back(q);
		s.pln = (int)b->pln_req.size() - 1;
	} else {
		b->pln_req[(size_t)s.pln] = q;
	}
	return MIJ_OK;
}

extern "C" int mij_batch_slot_plane_rect(const mij_batch *b, int slot, int comp, int rect[4])
{
	if (!rect || !batch_slot(b, slot) || comp < 0 || comp > 3)
		return set_err(MIJ_E_ARG, "mij_batch_slot_plane_rect: bad slot, component or destination");
	const Slot &s = b->slots[(size_t)slot];
	if (s.pln < 0)
		return set_err(MIJ_E_STATE, "mij_batch_slot_plane_rect: slot %d has no plane request", slot);
	const DevPlane &v = b->pln_req[(size_t)s.pln].dev.c[comp];
	if (!v.dst)
		return set_err(MIJ_E_ARG, "mij_batch_slot_plane_rect: component %d of slot %d is not wanted", comp, slot);
	rect[0] = (int)v.sx0, rect[1] = (int)v.sy0, rect[2] = (int)(v.sx1 - v.sx0), rect[3] = (int)(v.sy1 - v.sy0);
	return MIJ_OK;
}

extern "C" int mij_batch_timer_begin(mij_batch *b)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	HIP_TRY(hipSetDevice(b->ctx->device));
	HIP_TRY(hipEventRecord(b->ev_begin, b->stream));
	return MIJ_OK;
}
extern "C" int mij_batch_timer_end(mij_batch *b)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	HIP_TRY(hipSetDevice(b->ctx->device));
	HIP_TRY(hipEventRecord(b->ev_end, b->stream));
	return MIJ_OK;
}
extern "C" int mij_batch_timer_elapsed_ms(mij_batch *b, float *ms)
{
	if (!b || !ms)
		return set_err(MIJ_E_ARG, "bad argument");
	HIP_TRY(hipSetDevice(b->ctx->device));
	HIP_TRY(hipEventSynchronize(b->ev_end));
	HIP_TRY(hipEventElapsedTime(ms, b->ev_begin, b->ev_end));
	return MIJ_OK;
}

/* duration of k_pack_c8 (int16 staging -> compact planes) in the last mij_batch_upload, HIP events on the batch's stream; *ms = -1
 * when that upload packed nothing (every slot staged compact by the host walk, written by the GPU entropy stage, or int16 planes) */
extern "C" int mij_batch_pack_ms(mij_batch *b, float *ms)
{
	if (!b || !ms)
		return set_err(MIJ_E_ARG, "bad argument");
	*ms = -1.0f;
	if (!b->pack_timed)
		return MIJ_OK;
	HIP_TRY(hipSetDevice(b->ctx->device));
	HIP_TRY(hipEventSynchronize(b->ev_pack1));
	HIP_TRY(hipEventElapsedTime(ms, b->ev_pack0, b->ev_pack1));
	return MIJ_OK;
}

extern "C" int mij_batch_hash_out(mij_batch *b, int slot, uint64_t *hash)
{
	if (!hash || !batch_slot(b, slot))
		return set_err(MIJ_E_ARG, "bad argument");
	const Slot &s = b->slots[(size_t)slot];
	if (s.pln >= 0)
		return set_err(MIJ_E_STATE, "mij_batch_hash_out: slot %d has a plane request: it decodes no pixels", slot);
	if (wants_region(s))
		return set_err(MIJ_E_STATE, "mij_batch_hash_out: slot %d decodes a region only; the rest of its picture is unspecified", slot);
	const size_t bytes = out_px_bytes(s);
	std::vector<uint8_t> tmp(bytes);
	int rc = mij_batch_fetch(b, slot, tmp.data(), bytes);
	if (rc != MIJ_OK)
		return rc;
	uint64_t h = 1469598103934665603ull;
	for (size_t i = 0; i < bytes; ++i) {
		h ^= tmp[i];
		h *= 1099511628211ull;
	}
	*hash = h;
	return MIJ_OK;
}

/* words of 16 bytes in which two device images differ (parity checks of big batches: clones against their source) */
__global__ __launch_bounds__(256) void k_count_diff(const uint4 *__restrict__ a, const uint4 *__restrict__ b, uint32_t n, unsigned long long *__restrict__ out)
{
	uint32_t bad = 0;
	for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
		const uint4 x = a[i], y = b[i];
		bad += (x.x != y.x) | (x.y != y.y) | (x.z != y.z) | (x.w != y.w);
	}
	if (bad)
		atomicAdd(out, (unsigned long long)bad);
}

/* the last, partial 16-byte word of two reduced pictures: one more differing word when any of its n bytes differ */
__global__ __launch_bounds__(64) void k_count_diff_tail(const uint8_t *__restrict__ a, const uint8_t *__restrict__ b, uint32_t n, unsigned long long *__restrict__ out)
{
	const bool bad = threadIdx.x < n && a[threadIdx.x] != b[threadIdx.x];
	if (__builtin_amdgcn_ballot_w64(bad) != 0ull && threadIdx.x == 0)
		atomicAdd(out, 1ull);
}

extern "C" int mij_batch_diff_slots(mij_batch *b, const int *sa, const int *sb, int n, uint64_t *ndiff)
{
	if (!b || !sa || !sb || !ndiff || n < 0)
		return set_err(MIJ_E_ARG, "bad argument");
	if (!b->launched)
		return set_err(MIJ_E_STATE, "mij_batch_diff_slots before launch");
	HIP_TRY(hipSetDevice(b->ctx->device));
	Buf<unsigned long long, BUF_ON_DEVICE> cnt; /* freed on every way out (hipFree waits for the kernels queued so far) */
	unsigned long long h_cnt = 0;
	HIP_TRY(cnt.alloc(1));
	hipError_t e = hipMemsetAsync(cnt.d, 0, sizeof(unsigned long long), b->stream);
	for (int i = 0; i < n && e == hipSuccess; ++i) {
		if (!batch_slot(b, sa[i]) || !batch_slot(b, sb[i]))
			return set_err(MIJ_E_ARG, "bad slot pair %d", i);
		const Slot &x = b->slots[(size_t)sa[i]], &y = b->slots[(size_t)sb[i]];
		if (x.pln >= 0 || y.pln >= 0)
			return set_err(MIJ_E_STATE, "mij_batch_diff_slots: slot pair %d: a slot with a plane request decodes no pixels", i);
		if (wants_region(x) || wants_region(y))
			return set_err(MIJ_E_STATE, "mij_batch_diff_slots: slot pair %d: a slot that decodes a region only cannot be compared", i);
		/* a reduced picture leaves the rest of its region unwritten: its last, partial word is compared byte by byte */
		const bool exact = x.scale > 1 || y.scale > 1;
		const size_t px = out_px_bytes(x), bytes = exact ? px & ~(size_t)15 : align_up(px, 16);
		if (exact ? px != out_px_bytes(y) : bytes != align_up(out_px_bytes(y), 16))
			return set_err(MIJ_E_ARG, "slot pair %d: different sizes", i);
		if (exact && px > bytes)
			hipLaunchKernelGGL(k_count_diff_tail, dim3(1), dim3(64), 0, b->stream, b->out.d + x.dev.out_off + bytes, b->out.d + y.dev.out_off + bytes, (uint32_t)(px - bytes), cnt.d);
		/* outputs are 256-byte aligned and padded in the arena, so whole 16-byte words may be compared */
		hipLaunchKernelGGL(k_count_diff, dim3(1024), dim3(256), 0, b->stream, reinterpret_cast<const uint4 *>(b->out.d + x.dev.out_off),
								 reinterpret_cast<const uint4 *>(b->out.d + y.dev.out_off), (uint32_t)(bytes / 16), cnt.d);
		e = hipGetLastError();
	}
	if (e != hipSuccess) {
		(void)hipStreamSynchronize(b->stream);
		return set_err(MIJ_E_HIP, "mij_batch_diff_slots: %s", hipGetErrorString(e));
	}
	const int rc = d2h_bounced(b->ctx, b->stream, &h_cnt, cnt.d, sizeof(h_cnt));
	if (rc != MIJ_OK)
		return rc;
	*ndiff = (uint64_t)h_cnt;
	return MIJ_OK;
}

/* ------------------------------------------------------------------ GPU entropy stage (mij_batch_entropy_*): EsArena, above */

extern "C" int mij_batch_entropy_reserve(mij_batch *b, size_t stream_bytes)
{
	if (!b || !stream_bytes)
		return set_err(MIJ_E_ARG, "mij_batch_entropy_reserve: bad argument");
	if (b->es)
		return set_err(MIJ_E_STATE, "the entropy arena exists already");
	HIP_TRY(hipSetDevice(b->ctx->device));
	std::unique_ptr<EsArena> e(new (std::nothrow) EsArena());
	if (!e)
		return set_err(MIJ_E_NOMEM, "out of host memory");
	const size_t n = (size_t)b->max_images;
	const size_t stream_cap = align_up(stream_bytes + 64 * n, 256);
	e->scan_cap = 16 * n + 1024; /* restart intervals are walked one DevScan each */
	/* one picture per batch: short subsequences (latency), see MIJ_ES_BITS_SINGLE; MIJ_ES_BITS_OVERRIDE for experiments */
	e->sub_bits = n == 1 ? MIJ_ES_BITS_SINGLE : MIJ_ES_BITS;
	if (const char *env = getenv("MIJ_ES_BITS_OVERRIDE")) {
		const long v = atol(env);
		if (v >= 256 && v <= (long)MIJ_ES_BITS && (v & 31) == 0)
			e->sub_bits = (uint32_t)v;
	}
	/* shorter subsequences settle in more rounds; a round in which nothing moves costs a launch (~8 us), a look at the verdicts
	 * a wait: measured on one-picture batches, 1024 bits with 24 rounds queued up front is the quickest (profiles/r02v_single_call.json) */
	e->rounds0 = e->sub_bits >= 4096u ? 4 : (e->sub_bits >= 2048u ? 12 : (e->sub_bits >= 1024u ? 24 : 32));
	e->sub_cap = stream_cap * 8 / e->sub_bits + 2 * e->scan_cap;
	e->blk_cap = b->coef.cap / 128 + n;
	const size_t work_cap = e->sub_cap / MIJ_ES_WG + 2 * e->scan_cap, pack_cap = e->blk_cap / 256 + 8 * n;
	/* the write pass's intermediate form for compact planes: the record stream (mij_entropy_kernels.h) when its arena's record indices fit
	 * 32 bits (8 GiB: streams of about 1 GiB per batch) and MIJ_ES_RECORDS / the environment allow it, else the zigzag image */
	e->rec_region64 = (e->sub_bits + MIJ_ES_REC_SLACK) / 8u;
	e->rec_words = (e->sub_cap + 1) * (size_t)e->rec_region64;
	e->use_records = MIJ_ES_RECORDS && e->rec_words < ((size_t)1 << 30) && !(getenv("MIJ_ES_RECORDS") && getenv("MIJ_ES_RECORDS")[0] == '0');
	static_assert(sizeof(EsUni) % sizeof(uint4) == 0 && sizeof(EsW) % sizeof(uint4) == 0, "the table sets are read as uint4");
	hipError_t r = hipSuccess;
	auto get = [&r](auto &buf, size_t count) { /* in this order: the allocator sees the same sequence from every arena */
		if (r == hipSuccess)
			r = buf.alloc(count);
	};
	get(e->stream, stream_cap);
	get(e->scans, e->scan_cap);
	get(e->huff, 8 * n);
	get(e->work, work_cap);
	get(e->pack, pack_cap);
	get(e->start, e->sub_cap);
	get(e->end[0], e->sub_cap);
	get(e->end[1], e->sub_cap);
	get(e->uni, n * (sizeof(EsUni) / sizeof(uint4)));
	get(e->wtab, n * (sizeof(EsW) / sizeof(uint4)));
	get(e->tabscan, n);
	for (int q = 0; q < 2; ++q) {
		get(e->qidx[q], e->sub_cap);
		get(e->qstate[q], e->sub_cap);
	}
	get(e->cnt, e->sub_cap);
	get(e->base, e->sub_cap);
	get(e->meta, e->blk_cap);
	if (e->use_records)
		get(e->rec, e->rec_words);
	else
		get(e->zz, 64 * e->blk_cap);
	get(e->verdict, EV_ROWS * e->scan_cap);
	get(e->verdict_host, EV_ROWS * e->scan_cap);
	get(e->rounds_changed, (size_t)ES_MAX_ROUNDS);
	get(e->changed, ES_MAX_ROUNDS * e->scan_cap);
	if (r != hipSuccess) /* e goes, and what it got with it; b->es stays null */
		return set_err(r == hipErrorOutOfMemory ? MIJ_E_NOMEM : MIJ_E_HIP, "mij_batch_entropy_reserve: %s", hipGetErrorString(r));
	b->es = std::move(e);
	return MIJ_OK;
}

extern "C" uint8_t *mij_batch_entropy_stage(mij_batch *b, size_t *capacity)
{
	if (!b || !b->es)
		return nullptr;
	if (capacity)
		*capacity = b->es->stream.cap;
	return b->es->stream.h;
}

extern "C" int mij_batch_add_stream(mij_batch *b, const mjg_scan *scan, uint8_t *stream, size_t stream_len)
{
	if (!b || !b->es || !scan || !stream)
		return set_err(MIJ_E_ARG, "mij_batch_add_stream: bad argument (entropy arena reserved?)");
	EsArena *e = b->es.get();
	if (stream < e->stream.h || stream + stream_len + 32 > e->stream.h + e->stream.cap || ((size_t)(stream - e->stream.h) & 3u))
		return set_err(MIJ_E_ARG, "the stream must lie 4-byte aligned inside the pinned entropy region with 32 spare bytes behind it");
	if (scan->blocks_per_mcu < 1 || scan->blocks_per_mcu > 10 || scan->nblocks == 0 || stream_len >= (1u << 28))
		return set_err(MIJ_E_ARG, "bad scan description");
	/* the walk kernels compute plane addresses straight from these fields: they must describe the image's own MCU */
	{
		int rc = check_desc(&scan->desc);
		if (rc != MIJ_OK)
			return rc;
		const mij_image_desc &sd = scan->desc;
		uint32_t want = 0;
		for (int c = 0; c < sd.ncomp; ++c)
			want += (uint32_t)(sd.comp[c].h * sd.comp[c].v);
		if (want != scan->blocks_per_mcu || (uint64_t)scan->nblocks != (uint64_t)want * (uint32_t)sd.mcu_x * (uint32_t)sd.mcu_y)
			return set_err(MIJ_E_ARG, "scan block counts do not match the descriptor");
		for (uint32_t k = 0; k < scan->blocks_per_mcu; ++k) {
			const uint32_t ci = scan->blk_comp[k];
			if (ci >= (uint32_t)sd.ncomp || scan->blk_dx[k] >= (uint32_t)sd.comp[ci].h || scan->blk_dy[k] >= (uint32_t)sd.comp[ci].v)
				return set_err(MIJ_E_ARG, "scan block %u lies outside its component's MCU", k);
		}
		for (int c = 0; c < sd.ncomp; ++c)
			if (scan->dc_tab[c] > 3 || scan->ac_tab[c] < 4 || scan->ac_tab[c] > 7)
				return set_err(MIJ_E_ARG, "bad Huffman table index for component %d", c);
		/* blocks of an MCU in the order of the interleaved scan (codec/jpeg.c:1204-1219): component, then row, then column */
		uint32_t k = 0;
		for (int c = 0; c < sd.ncomp; ++c)
			for (int y = 0; y < sd.comp[c].v; ++y)
				for (int x = 0; x < sd.comp[c].h; ++x, ++k)
					if (scan->blk_comp[k] != c || scan->blk_dx[k] != x || scan->blk_dy[k] != y)
						return set_err(MIJ_E_ARG, "scan block %u is not in interleaved-scan order", k);
	}
	size_t need_pack = 0;
	for (int c = 0; c < scan->desc.ncomp; ++c)
		need_pack += (comp_tiles(scan->desc.comp[c]) * 64 + 255) / 256;
	if (b->coef_fmt && b->es->pack_used + need_pack > b->es->pack.cap)
		return set_err(MIJ_E_NOMEM, "entropy arena exhausted");
	/* one DevScan per restart interval (one for the whole stream without restart markers) */
	const uint32_t nseg = scan->n_seg ? scan->n_seg : 1u;
	if ((size_t)scan->seg_table_off + 8u * (size_t)nseg > stream_len || (scan->seg_table_off & 3u))
		return set_err(MIJ_E_ARG, "bad segment table");
	const uint32_t *table = reinterpret_cast<const uint32_t *>(stream + scan->seg_table_off);
	const uint32_t nmcu = scan->nblocks / scan->blocks_per_mcu;
	size_t need_sub = 0, need_work = 0;
	for (uint32_t g = 0; g < nseg; ++g) {
		const size_t off = table[2 * g], len = table[2 * g + 1];
		if ((off & 3u) || off + len + 32 > stream_len + 32 || off + len > scan->seg_table_off)
			return set_err(MIJ_E_ARG, "bad segment %u", g);
		const size_t ns = (len * 8 + e->sub_bits - 1) / e->sub_bits;
		need_sub += ns ? ns : 1;
		need_work += (ns ? ns : 1) / MIJ_ES_WG + 1;
	}
	if (scan->n_seg && ((uint64_t)scan->restart_mcus * (nseg - 1) >= nmcu || (uint64_t)scan->restart_mcus * nseg < nmcu))
		return set_err(MIJ_E_ARG, "segment count does not match the restart interval");
	if (e->sub_used + need_sub > e->sub_cap || e->blk_used + scan->nblocks > e->blk_cap || e->work_used + need_work > e->work.cap ||
		 e->scan_slot.size() + nseg > e->scan_cap || e->n_tabs + 1 > (size_t)b->max_images)
		return set_err(MIJ_E_NOMEM, "entropy arena exhausted");
	const int slot = add_common(b, &scan->desc, -1, true);
	if (slot < 0)
		return slot;
	Slot &s = b->slots[(size_t)slot];
	s.dev_coef = 1;
	s.es_index = (int)e->scan_slot.size();
	/* The walk writes the batch's plane format straight into HBM: compact planes by default (every decode kernel
	 * reads them; a coefficient outside -128..127 becomes an escape byte, nothing is handed back for its size),
	 * int16 tile layout on request (mij_batch_set_coef_format). */
	s.coef_bytes_fmt = b->coef_fmt ? 1 : 0;
	layout_coef(s);
	if (s.coef_bytes_fmt)
		for (int c = 0; c < scan->desc.ncomp; ++c)
			for (uint32_t f = 0, nb = (uint32_t)comp_tiles(scan->desc.comp[c]) * 64u; f < nb; f += 256) {
				WorkIdct w = {(uint32_t)slot, (uint32_t)c, f, 0u};
				e->pack.h[e->pack_used++] = w;
			}
	s.dev.es_blk_off = (uint32_t)e->blk_used;
	s.dev.es_bpm = (uint8_t)scan->blocks_per_mcu;
	for (int c = 0, j = 0; c < scan->desc.ncomp; ++c) {
		s.dev.es_j0[c] = (uint8_t)j;
		j += scan->desc.comp[c].h * scan->desc.comp[c].v;
	}
	static_assert(sizeof(DevHuff) == sizeof(mjg_huff), "mjg_huff and DevHuff must match");
	const size_t tab = e->n_tabs++;
	memcpy(&e->huff.h[8 * tab], scan->huff, sizeof(mjg_huff) * 8);
	e->tabscan.h[tab] = (uint32_t)e->scan_slot.size(); /* the first of this picture's scans */
	uint32_t first_mcu = 0;
	for (uint32_t g = 0; g < nseg; ++g) {
		const size_t k = e->scan_slot.size();
		const size_t off = table[2 * g], len = table[2 * g + 1];
		const uint32_t seg_mcus = scan->n_seg ? (g + 1 < nseg ? scan->restart_mcus : nmcu - first_mcu) : nmcu;
		const size_t ns = (len * 8 + e->sub_bits - 1) / e->sub_bits;
		DevScan &d = e->scans.h[k];
		memset(&d, 0, sizeof(d));
		d.stream_off = (uint64_t)(stream - e->stream.h) + off;
		d.nbits = (uint32_t)(len * 8);
		d.nsub = (uint32_t)(ns ? ns : 1);
		d.sub_off = (uint32_t)e->sub_used;
		d.img = (uint32_t)slot;
		d.nblocks = seg_mcus * scan->blocks_per_mcu;
		d.blk_off = (uint32_t)e->blk_used;
		d.bpm = scan->blocks_per_mcu;
		d.mcu_x = (uint32_t)scan->desc.mcu_x;
		d.first_mcu = first_mcu;
		d.last_seg = g + 1 == nseg;
		d.fmt = (uint32_t)s.coef_bytes_fmt;
		memcpy(d.blk_comp, scan->blk_comp, 12);
		memcpy(d.blk_dx, scan->blk_dx, 12);
		memcpy(d.blk_dy, scan->blk_dy, 12);
		memcpy(d.dc_tab, scan->dc_tab, 4);
		memcpy(d.ac_tab, scan->ac_tab, 4);
		d.tab_off = (uint32_t)(8 * tab);
		d.sub_bits = e->sub_bits;
		memcpy(d.qz, scan->qz, sizeof(d.qz));
		for (uint32_t f = 0; f < d.nsub; f += MIJ_ES_WG) {
			EsWork w = {(uint32_t)k, f};
			e->work.h[e->work_used++] = w;
		}
		e->sub_used += d.nsub;
		e->blk_used += d.nblocks;
		e->scan_slot.push_back(slot);
		first_mcu += seg_mcus;
	}
	return slot;
}

/* everything after the synchronisation rounds: offsets, write, tails, DC, verdict D2H (asynchronous) */
static int es_enqueue_tail(mij_batch *b)
{
	EsArena *e = b->es.get();
	hipStream_t st = b->stream;
	const size_t ns = e->scan_slot.size();
	/* the counters of the last round queued so far (slice 0 is clear when there was none) */
	uint32_t *v_anom = e->d_row(EV_ANOMALY), *v_changed = e->changed.d + (size_t)(e->last_rounds > 0 ? e->last_rounds - 1 : 0) * e->scan_cap, *v_total = e->d_row(EV_TOTAL),
				*v_l1 = e->d_row(EV_L1MAX), *v_pfinal = e->d_row(EV_PFINAL);
	const dim3 gw((unsigned)e->work_used), gs((unsigned)ns), blk(256), wblk(MIJ_ES_WG);
	hipLaunchKernelGGL(k_es_offsets, gs, blk, 0, st, e->scans.d, e->cnt.d, e->base.d, v_total);
	HIP_TRY(hipGetLastError());
	{
		/* compact planes: the write pass fills a cleared intermediate image (k_es_pack then writes every byte of the
		 * tiles, k_es_dc the DC array, the first escape of a block clears its escape bytes: the planes themselves need
		 * no clearing).  int16 planes: the write pass only stores non-zero coefficients, so the planes of those images
		 * are cleared (neighbours in the arena as one range). */
		if (e->pack_used && !e->use_records)
			HIP_TRY(hipMemsetAsync(e->zz.d, 0, 64 * e->blk_used, st));
		if (e->pack_used && e->use_records) /* record form: "no subsequence began this block" until the write pass says where its records start */
			HIP_TRY(hipMemsetAsync(e->meta.d, 0xff, sizeof(uint64_t) * e->blk_used, st));
		size_t lo = 0, hi = 0;
		for (const Slot &sl : b->slots) {
			if (!sl.dev_coef || sl.clone_of >= 0 || sl.coef_bytes_fmt)
				continue;
			const size_t a = sl.coef_base, z = a + sl.coef_bytes;
			if (a == hi && hi > lo) {
				hi = z;
				continue;
			}
			if (hi > lo)
				HIP_TRY(hipMemsetAsync(b->coef.d + lo, 0, hi - lo, st));
			lo = a;
			hi = z;
		}
		if (hi > lo)
			HIP_TRY(hipMemsetAsync(b->coef.d + lo, 0, hi - lo, st));
		/* one launch per plane format in use (the other kind's workgroups leave at once) */
		bool any_fmt[2] = {false, false};
		for (size_t k = 0; k < ns; ++k)
			any_fmt[e->scans.h[k].fmt ? 1 : 0] = true;
		if (any_fmt[1] && e->use_records)
			hipLaunchKernelGGL(k_es_writer, gw, wblk, 0, st, e->scans.d, e->work.d, e->huff.d, e->stream.d, e->start.d, e->base.d, e->meta.d, v_anom, v_pfinal, e->rec.d,
									 e->rec_region64, e->wtab.d);
		else if (any_fmt[1])
			hipLaunchKernelGGL(k_es_write<true>, gw, wblk, 0, st, e->scans.d, e->work.d, e->huff.d, e->stream.d, b->imgs.d, e->start.d, e->base.d,
									 reinterpret_cast<int16_t *>(b->coef.d), e->meta.d, v_anom, v_pfinal, e->zz.d);
		if (any_fmt[0])
			hipLaunchKernelGGL(k_es_write<false>, gw, wblk, 0, st, e->scans.d, e->work.d, e->huff.d, e->stream.d, b->imgs.d, e->start.d, e->base.d,
									 reinterpret_cast<int16_t *>(b->coef.d), e->meta.d, v_anom, v_pfinal, e->zz.d);
		HIP_TRY(hipGetLastError());
		if (any_fmt[1] && !e->use_records)
			hipLaunchKernelGGL(k_es_tails<true>, gw, wblk, 0, st, e->scans.d, e->work.d, e->huff.d, e->stream.d, b->imgs.d, e->start.d, e->base.d,
									 reinterpret_cast<int16_t *>(b->coef.d), e->meta.d, e->rounds_changed.d, e->zz.d);
		if (any_fmt[0])
			hipLaunchKernelGGL(k_es_tails<false>, gw, wblk, 0, st, e->scans.d, e->work.d, e->huff.d, e->stream.d, b->imgs.d, e->start.d, e->base.d,
									 reinterpret_cast<int16_t *>(b->coef.d), e->meta.d, e->rounds_changed.d, e->zz.d);
	}
	HIP_TRY(hipGetLastError());
	if (e->pack_used) {
		if (e->use_records)
			hipLaunchKernelGGL(k_es_pack2, dim3((unsigned)e->pack_used), blk, 0, st, b->imgs.d, e->pack.d, e->rec.d, (uint32_t)e->rec_words, b->coef.d, e->meta.d);
		else
			hipLaunchKernelGGL(k_es_pack, dim3((unsigned)e->pack_used), blk, 0, st, b->imgs.d, e->pack.d, e->zz.d, b->coef.d, e->meta.d);
		HIP_TRY(hipGetLastError());
	}
	hipLaunchKernelGGL(k_es_dc, gs, blk, 0, st, e->scans.d, b->imgs.d, v_total, v_changed, reinterpret_cast<int16_t *>(b->coef.d), e->meta.d,
							 v_anom, v_l1, v_pfinal, e->stream.d);
	HIP_TRY(hipGetLastError());
	/* only the words of this batch's scans: five short runs */
	for (int v = 0; v < EV_ROWS; ++v)
		HIP_TRY(copy_table_to_host(e->h_row((EsVerdict)v), v == EV_CHANGED ? v_changed : e->d_row((EsVerdict)v), sizeof(uint32_t) * ns, st));
	return MIJ_OK;
}

static int es_enqueue_round(mij_batch *b)
{
	EsArena *e = b->es.get();
	hipStream_t st = b->stream;
	if (e->last_rounds >= ES_MAX_ROUNDS)
		return set_err(MIJ_E_STATE, "too many synchronisation rounds");
	uint32_t *v_changed = e->changed.d + (size_t)e->last_rounds * e->scan_cap; /* this round's slice, cleared by the launch */
	const dim3 gw((unsigned)e->work_used), blk(MIJ_ES_WG);
	/* v_changed: what this round leaves for the next one (0 everywhere: the chains have settled) */
	const int r = e->last_rounds;
	if (r == 0)
		hipLaunchKernelGGL(k_es_sync, gw, blk, 0, st, e->scans.d, e->work.d, e->huff.d, e->stream.d, e->start.d, e->end[0].d, e->end[1].d, e->cnt.d, v_changed, e->qidx[0].d,
								 e->qstate[0].d, e->uni.d);
	else
		hipLaunchKernelGGL(k_es_syncq, gw, blk, 0, st, e->scans.d, e->work.d, e->huff.d, e->stream.d, e->start.d, e->end[1].d, e->cnt.d, v_changed - e->scan_cap,
								 e->qidx[(r - 1) & 1].d, e->qstate[(r - 1) & 1].d, v_changed, e->qidx[r & 1].d, e->qstate[r & 1].d, e->uni.d);
	HIP_TRY(hipGetLastError());
	++e->last_rounds;
	return MIJ_OK;
}

/* Asynchronous: uploads, cold pass, a fixed number of synchronisation rounds (enough for ordinary pictures),
 * write / DC passes and the verdict copy are queued on the batch's stream; nothing waits. */
extern "C" int mij_batch_entropy_launch(mij_batch *b)
{
	if (!b || !b->es)
		return set_err(MIJ_E_ARG, "mij_batch_entropy_launch: bad argument");
	EsArena *e = b->es.get();
	const size_t ns = e->scan_slot.size();
	e->in_flight = false;
	if (!ns)
		return MIJ_OK;
	HIP_TRY(hipSetDevice(b->ctx->device));
	hipStream_t st = b->stream;
	const size_t n = b->slots.size();
	for (size_t i = 0; i < n; ++i)
		b->imgs.h[i] = b->slots[i].dev;
	HIP_TRY(copy_table(b->imgs.d, b->imgs.h, sizeof(DevImage) * n, st));
	HIP_TRY(copy_table(e->scans.d, e->scans.h, sizeof(DevScan) * ns, st));
	HIP_TRY(copy_table(e->huff.d, e->huff.h, sizeof(DevHuff) * 8 * e->n_tabs, st));
	HIP_TRY(copy_table(e->tabscan.d, e->tabscan.h, sizeof(uint32_t) * e->n_tabs, st));
	HIP_TRY(copy_table(e->work.d, e->work.h, sizeof(EsWork) * e->work_used, st));
	HIP_TRY(copy_table(e->pack.d, e->pack.h, sizeof(WorkIdct) * e->pack_used, st));
	/* streams: one copy from the first to the last byte in use */
	size_t lo = (size_t)-1, hi = 0;
	for (size_t k = 0; k < ns; ++k) {
		const DevScan &d = e->scans.h[k];
		lo = d.stream_off < lo ? (size_t)d.stream_off : lo;
		const size_t end = (size_t)d.stream_off + d.nbits / 8 + 32;
		hi = end > hi ? end : hi;
	}
	/* The copy engine, not the copy kernel: measured both ways with four walks in flight (profiles/r02n): through
	 * k_copy_words16 the call never blocks but the 58 MB cross PCIe under a kernel that holds workgroup slots (78 Gpix/s end
	 * to end); hipMemcpyAsync blocks the host for ~7 ms one call in three or four and still comes out ahead (100 Gpix/s). */
	HIP_TRY(hipMemcpyAsync(e->stream.d + lo, e->stream.h + lo, hi - lo, hipMemcpyHostToDevice, st));
	/* the write pass stores every block of the MCU grid whole and its L1 word with it, so neither the
	 * coefficient planes nor the accumulators need clearing; the verdicts do */
	HIP_TRY(hipMemsetAsync(e->verdict.d, 0, sizeof(uint32_t) * EV_ROWS * e->scan_cap, st));
	HIP_TRY(hipMemsetAsync(e->changed.d, 0, sizeof(uint32_t) * ES_MAX_ROUNDS * e->scan_cap, st));
	const dim3 gw((unsigned)e->work_used), blk(MIJ_ES_WG);
	hipLaunchKernelGGL(k_es_tables, dim3((unsigned)e->n_tabs), dim3(256), 0, st, e->scans.d, e->tabscan.d, e->huff.d, e->uni.d, e->wtab.d);
	HIP_TRY(hipGetLastError());
	hipLaunchKernelGGL(k_es_cold, gw, blk, 0, st, e->scans.d, e->work.d, e->huff.d, e->stream.d, e->start.d, e->end[0].d, e->cnt.d, e->uni.d);
	HIP_TRY(hipGetLastError());
	e->last_rounds = 0;
	int rounds = e->rounds0; /* 4096-bit subsequences: ordinary pictures settle in two or three of four; finish() adds rounds for those that have not */
	if (const char *env = getenv("MIJ_ES_ROUNDS"))
		rounds = atoi(env) > 0 && atoi(env) <= ES_MAX_ROUNDS ? atoi(env) : rounds;
	for (int r = 0; r < rounds; ++r) {
		int rc = es_enqueue_round(b);
		if (rc != MIJ_OK)
			return rc;
	}
	int rc = es_enqueue_tail(b);
	if (rc != MIJ_OK)
		return rc;
	e->in_flight = true;
	return MIJ_OK;
}

/* Waits for mij_batch_entropy_launch.  Images whose chains had not settled get more rounds (stopping as soon as
 * a round moves nothing, ES_MAX_ROUNDS at most) and the write / DC passes are repeated; then the verdicts. */
extern "C" int mij_batch_entropy_finish(mij_batch *b, int *fallback, int cap, int *n_fallback)
{
	if (!b || !b->es || !n_fallback)
		return set_err(MIJ_E_ARG, "mij_batch_entropy_finish: bad argument");
	EsArena *e = b->es.get();
	*n_fallback = 0;
	const size_t ns = e->scan_slot.size();
	if (!ns || !e->in_flight)
		return MIJ_OK;
	e->in_flight = false;
	HIP_TRY(hipSetDevice(b->ctx->device));
	hipStream_t st = b->stream;
	HIP_TRY(hipStreamSynchronize(st));
	bool unsettled = false;
	for (size_t k = 0; k < ns; ++k)
		unsettled |= (e->h_row(EV_ANOMALY)[k] & 8u) != 0;
	if (unsettled) {
		while (e->last_rounds < ES_MAX_ROUNDS) {
			int rc = MIJ_OK;
			for (int r = 0; r < 4 && e->last_rounds < ES_MAX_ROUNDS && rc == MIJ_OK; ++r)
				rc = es_enqueue_round(b);
			if (rc != MIJ_OK)
				return rc;
			HIP_TRY(hipMemcpyAsync(e->h_row(EV_CHANGED), e->changed.d + (size_t)(e->last_rounds - 1) * e->scan_cap, sizeof(uint32_t) * ns, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipStreamSynchronize(st));
			uint32_t any = 0;
			for (size_t k = 0; k < ns; ++k)
				any |= e->h_row(EV_CHANGED)[k];
			if (!any)
				break;
		}
		/* the passes behind the rounds again, on clean verdicts (the last round's counters stay) */
		HIP_TRY(hipMemsetAsync(e->d_row(EV_ANOMALY), 0, sizeof(uint32_t) * e->scan_cap, st));
		HIP_TRY(hipMemsetAsync(e->d_row(EV_TOTAL), 0, sizeof(uint32_t) * (EV_ROWS - EV_TOTAL) * e->scan_cap, st));
		int rc = es_enqueue_tail(b);
		if (rc != MIJ_OK)
			return rc;
		HIP_TRY(hipStreamSynchronize(st));
	}
	if (getenv("MIJ_ES_DEBUG"))
		for (size_t k = 0; k < ns; ++k)
			fprintf(stderr, "es scan %zu slot %d: anomaly %u changed %u blocks %u/%u l1max %u nsub %u rounds %d\n", k, e->scan_slot[k], e->h_row(EV_ANOMALY)[k],
					  e->h_row(EV_CHANGED)[k], e->h_row(EV_TOTAL)[k], e->scans.h[k].nblocks, e->h_row(EV_L1MAX)[k], e->scans.h[k].nsub, e->last_rounds);
	/* a slot's restart intervals are consecutive scans: any verdict bit in one of them hands the image back */
	for (size_t k = 0; k < ns;) {
		const int slot = e->scan_slot[k];
		uint32_t bad = 0, l1max = 0;
		for (; k < ns && e->scan_slot[k] == slot; ++k) {
			bad |= e->h_row(EV_ANOMALY)[k];
			const uint32_t v = e->h_row(EV_L1MAX)[k];
			l1max = v > l1max ? v : l1max;
		}
		Slot &s = b->slots[(size_t)slot];
		if (bad) {
			if (*n_fallback < cap && fallback)
				fallback[*n_fallback] = slot;
			++*n_fallback;
			continue;
		}
		if (l1max > MIJ_BLOCK_L1_LIMIT)
			s.desc.flags |= MIJ_FLAG_WIDE_IDCT;
	}
	b->uploaded = b->launched = false;
	if (*n_fallback > cap)
		return set_err(MIJ_E_ARG, "fallback list too small (%d > %d)", *n_fallback, cap);
	return MIJ_OK;
}

extern "C" int mij_batch_entropy_run(mij_batch *b, int *fallback, int cap, int *n_fallback)
{
	int rc = mij_batch_entropy_launch(b);
	if (rc != MIJ_OK)
		return rc;
	return mij_batch_entropy_finish(b, fallback, cap, n_fallback);
}

extern "C" int mij_batch_entropy_anomaly(mij_batch *b, int slot)
{
	if (!batch_slot(b, slot) || !b->es)
		return set_err(MIJ_E_ARG, "mij_batch_entropy_anomaly: bad argument");
	const EsArena *e = b->es.get();
	if (e->in_flight)
		return set_err(MIJ_E_ARG, "mij_batch_entropy_anomaly: the walk has not been finished");
	uint32_t bad = 0;
	bool found = false;
	for (size_t k = 0; k < e->scan_slot.size(); ++k)
		if (e->scan_slot[k] == slot) {
			bad |= e->h_row(EV_ANOMALY)[k];
			found = true;
		}
	if (!found)
		return set_err(MIJ_E_ARG, "slot %d was not walked on the GPU", slot);
	return (int)(bad & 0x7fffffffu);
}

extern "C" int mij_batch_fallback_prepare(mij_batch *b, int slot)
{
	if (!batch_slot(b, slot))
		return MIJ_E_ARG;
	Slot &s = b->slots[(size_t)slot];
	if (!s.dev_coef)
		return MIJ_OK;
	if (s.stage_off == MIJ_NO_STAGE)
		return set_err(MIJ_E_NOMEM, "slot %d has no staging planes (the staging arena was too small when it was added)", slot);
	s.dev_coef = 0;
	s.coef_bytes_fmt = 0; /* staged as int16 by the host walk; upload decides the format in HBM */
	layout_coef(s);
	s.desc.flags &= ~(uint32_t)MIJ_FLAG_WIDE_IDCT;
	memset(b->stage.h + s.stage_off, 0, s.coef_bytes);
	b->uploaded = b->launched = false;
	return MIJ_OK;
}

extern "C" int mij_batch_fetch_coef(mij_batch *b, int slot, int16_t *dst, size_t dst_elems)
{
	if (!dst || !batch_slot(b, slot))
		return set_err(MIJ_E_ARG, "bad slot or destination");
	const Slot &s = b->slots[(size_t)slot];
	size_t elems = 0;
	for (int c = 0; c < s.desc.ncomp; ++c)
		elems += comp_tiles(s.desc.comp[c]) << 12;
	if (dst_elems < elems)
		return set_err(MIJ_E_ARG, "destination too small");
	HIP_TRY(hipSetDevice(b->ctx->device));
	if (!s.coef_bytes_fmt) {
		return d2h_bounced(b->ctx, b->stream, dst, b->coef.d + s.coef_base, elems * sizeof(int16_t));
	}
	/* compact planes: bring the region over and expand it on the host into the int16 tile layout */
	std::vector<uint8_t> raw(s.coef_bytes);
	{
		const int rc = d2h_bounced(b->ctx, b->stream, raw.data(), b->coef.d + s.coef_base, s.coef_bytes);
		if (rc != MIJ_OK)
			return rc;
	}
	size_t eoff = 0;
	for (int c = 0; c < s.desc.ncomp; ++c) {
		const size_t nt = comp_tiles(s.desc.comp[c]);
		size_t lo_o, dc_o, hi_o;
		mij_compact_offsets(&s.desc, c, &lo_o, &dc_o, &hi_o);
		const uint8_t *lo = raw.data() + lo_o, *dcp = raw.data() + dc_o, *hi = raw.data() + hi_o;
		int16_t *out = dst + eoff;
		for (size_t L = 0; L < nt * 64; ++L) {
			const uint8_t *blo = lo + ((L >> 6) << 12) + ((L & 63) << 3);
			int16_t *bo = out + ((L >> 6) << 12) + ((L & 63) << 3);
			const bool esc = (blo[0] & 1u) != 0;
			for (int P = 0; P < 64; ++P) {
				int v = (int8_t)blo[((size_t)(P >> 3) << 9) + (P & 7)];
				if (esc)
					v += 256 * (int)hi[(L << 6) + P];
				bo[((size_t)(P >> 3) << 9) + (P & 7)] = (int16_t)v;
			}
			uint16_t dcv;
			memcpy(&dcv, dcp + 2 * L, 2);
			bo[0] = (int16_t)dcv;
		}
		eoff += nt << 12;
	}
	return MIJ_OK;
}

extern "C" int mij_batch_set_coef_format(mij_batch *b, int fmt)
{
	if (!b || (fmt != MIJ_COEF_INT16 && fmt != MIJ_COEF_COMPACT))
		return set_err(MIJ_E_ARG, "bad coefficient format");
	b->coef_fmt = fmt;
	b->uploaded = b->launched = false;
	return MIJ_OK;
}

extern "C" int mij_batch_slot_escapes(mij_batch *b, int slot)
{
	if (!batch_slot(b, slot))
		return MIJ_E_ARG;
	const Slot &s = b->slots[(size_t)slot];
	if (!s.coef_bytes_fmt)
		return 0;
	HIP_TRY(hipSetDevice(b->ctx->device));
	int total = 0;
	for (int c = 0; c < s.desc.ncomp; ++c) {
		const size_t nt = comp_tiles(s.desc.comp[c]);
		std::vector<uint8_t> lo(nt << 12);
		{
			const int rc = d2h_bounced(b->ctx, b->stream, lo.data(), b->coef.d + s.dev.comp[c].coef_off, nt << 12);
			if (rc != MIJ_OK)
				return rc;
		}
		for (size_t L = 0; L < (size_t)(s.desc.comp[c].bw * s.desc.comp[c].bh); ++L)
			total += lo[((L >> 6) << 12) + ((L & 63) << 3)] & 1;
	}
	return total;
}

/* Measurement: how many wavefronts of the decode kernels took which sparse-block transform (mij_kernels.h, "sparse blocks").  With
 * on != 0 every image descriptor of the uploaded batch gets MIJ_DEV_COUNT_CLASSES and the device counters are cleared; the launches
 * that follow add to them; mij_batch_idct_class_counts waits for the stream and reads them.  Off by default: the timed launches of
 * bench.py run without it. */
extern "C" int mij_batch_count_idct_classes(mij_batch *b, int on)
{
	if (!b)
		return set_err(MIJ_E_ARG, "batch is NULL");
	if (!b->uploaded)
		return set_err(MIJ_E_STATE, "mij_batch_count_idct_classes before mij_batch_upload");
	HIP_TRY(hipSetDevice(b->ctx->device));
	HIP_TRY(hipStreamSynchronize(b->stream));
	const size_t n = b->slots.size();
	for (size_t i = 0; i < n; ++i) {
		if (on)
			b->imgs.h[i].flags |= MIJ_DEV_COUNT_CLASSES;
		else
			b->imgs.h[i].flags &= ~(int32_t)MIJ_DEV_COUNT_CLASSES;
	}
	HIP_TRY(copy_table(b->imgs.d, b->imgs.h, sizeof(DevImage) * n, b->stream));
	if (on) {
		void *sym = nullptr;
		HIP_TRY(hipGetSymbolAddress(&sym, HIP_SYMBOL(g_idct_class)));
		HIP_TRY(hipMemsetAsync(sym, 0, sizeof(unsigned long long) * 4, b->stream));
	}
	HIP_TRY(hipStreamSynchronize(b->stream));
	return MIJ_OK;
}

extern "C" int mij_batch_idct_class_counts(mij_batch *b, uint64_t out[4])
{
	if (!b || !out)
		return set_err(MIJ_E_ARG, "bad argument");
	HIP_TRY(hipSetDevice(b->ctx->device));
	void *sym = nullptr;
	HIP_TRY(hipGetSymbolAddress(&sym, HIP_SYMBOL(g_idct_class)));
	unsigned long long v[4];
	const int rc = d2h_bounced(b->ctx, b->stream, v, sym, sizeof(v));
	if (rc != MIJ_OK)
		return rc;
	for (int i = 0; i < 4; ++i)
		out[i] = v[i];
	return MIJ_OK;
}

extern "C" int mij_batch_slot_coef_bytes(const mij_batch *b, int slot)
{
	if (!batch_slot(b, slot))
		return 0;
	return b->slots[(size_t)slot].coef_bytes_fmt;
}

extern "C" int mij_batch_entropy_rounds(const mij_batch *b) { return b && b->es ? b->es->last_rounds : 0; }

/* ------------------------------------------------------------------ encoder (mij_enc_*)
 *
 * GPU half of the JPEG writer: colour transform + 2x2 chroma mean + float AAN fDCT + quantiser
 * (codec/jpeg_write.c:24-118, :283-352) for a batch of images; the host then Huffman-codes the data
 * units (mjw_emit, mij_host.h), or, with an emission arena, the GPU does (mij_emit_kernels.h).  Same arena / stream /
 * work-list design as the decode batch.
 */
#include "mij_host.h"
#include "mij_emit_kernels.h"
#include "mij_transcode_kernels.h"
#include "mij_libjpeg_enc_kernels.h"
static_assert(MIJ_EMIT_HDR == MJW_LJ_HEADER_BYTES, "header size");

/* where a slot's input comes from: pinned staging, a device tensor, given units, a decode batch's coefficient planes */
enum EncKind { ENC_HOST = 0, ENC_DEVICE = 1, ENC_UNITS = 2, ENC_COEF = 3 };
static inline bool enc_has_pixels(EncKind kind) { return kind == ENC_HOST || kind == ENC_DEVICE; }

/* The transform kernels, in launch order: the per-unit luma / chroma pairs of 4:4:4 and 4:2:0 (the strip kernels' test twins,
 * mij_enc_force_generic), the strip kernels of pixel slots, the strip kernels of plane slots.  Every one takes (slots, work, pixel arena,
 * unit arena).  A work item is `strip` consecutive MCUs of one slot; of the per-unit pairs, 256 units of one kind. */
enum EncGroup {
	EG_NONE = -1, EG_Y444 = 0, EG_C444, EG_Y420, EG_C420, EG_420, EG_444, EG_422, EG_440, EG_GREY, EG_P444, EG_P422, EG_P440, EG_P420, EG_PGREY,
	/* libjpeg slots (mij_enc_set_arith; mij_libjpeg_enc_kernels.h): pass 1 of the pixel slots, then pass 2 of pixel and plane slots alike */
	EG_LJC444, EG_LJC422, EG_LJC420, EG_LJCGREY, EG_LJ444, EG_LJ422, EG_LJ420, EG_LJGREY,
	EG_GROUPS
};
static_assert(EG_GROUPS == MIJ_ENC_GROUPS, "mij.h names the groups");
#define EG_LJ_PASS1(g) ((EncGroup)((g) - (EG_LJ444 - EG_LJC444))) /* the colour pass in front of transform group g */
typedef void (*enc_lj_fn)(const EncImage *, const WorkIdct *, const uint8_t *, int16_t *, const LjEncSlot *, uint8_t *);
struct EncFamily {
	void (*k)(const EncImage *, const WorkIdct *, const uint8_t *, int16_t *);
	unsigned threads; /* workgroup size */
	size_t lds;       /* dynamic LDS bytes */
	uint32_t strip;
	enc_lj_fn klj; /* a libjpeg family's kernel instead of k: it also takes the slots' LjEncSlot list and the plane scratch */
};
#define MIJ_ENCP(LH, LV, NC) {k_encode_planes<LH, LV, NC>, MIJ_ENCP_NT(LH, LV, NC), MIJ_ENCP_LDS(LH, LV, NC), MIJ_ENCP_STRIP(LH, LV, NC), nullptr}
/* pass 1: an item is one row of cells (8 mcu_y of them); pass 2: k_encode_planes' strips */
#define MIJ_LJC(LH, LV, NC) {nullptr, 256, 0, 1, k_lj_enc_color<LH, LV, NC>}
#define MIJ_LJP(LH, LV, NC) {nullptr, MIJ_ENCP_NT(LH, LV, NC), MIJ_ENCP_LDS(LH, LV, NC), MIJ_ENCP_STRIP(LH, LV, NC), k_lj_encode_planes<LH, LV, NC>}
static const EncFamily enc_families[EG_GROUPS] = {
	/* EG_Y444 */ {k_encode_y<0>, 256, 0, 256, nullptr},
	/* EG_C444 */ {k_encode_c<0>, 256, 0, 256, nullptr},
	/* EG_Y420 */ {k_encode_y<1>, 256, 0, 256, nullptr},
	/* EG_C420 */ {k_encode_c<1>, 256, 0, 256, nullptr},
	/* EG_420 */ {k_encode420, 192, MIJ_ENC_LDS, MIJ_ENC_STRIP, nullptr},
	/* EG_444 */ {k_encode444, 192, MIJ_ENC444_LDS, MIJ_ENC444_STRIP, nullptr},
	/* EG_422 */ {k_encode422, 128, MIJ_ENC422_LDS, MIJ_ENC422_STRIP, nullptr},
	/* EG_440 */ {k_encode440, 256, MIJ_ENC440_LDS, MIJ_ENC440_STRIP, nullptr},
	/* EG_GREY */ {k_encode_grey, 256, MIJ_ENCGREY_LDS, MIJ_ENCGREY_STRIP, nullptr},
	/* EG_P444 */ MIJ_ENCP(1, 1, 3),
	/* EG_P422 */ MIJ_ENCP(2, 1, 3),
	/* EG_P440 */ MIJ_ENCP(1, 2, 3),
	/* EG_P420 */ MIJ_ENCP(2, 2, 3),
	/* EG_PGREY */ MIJ_ENCP(1, 1, 1),
	/* EG_LJC444 */ MIJ_LJC(1, 1, 3),
	/* EG_LJC422 */ MIJ_LJC(2, 1, 3),
	/* EG_LJC420 */ MIJ_LJC(2, 2, 3),
	/* EG_LJCGREY */ MIJ_LJC(1, 1, 1),
	/* EG_LJ444 */ MIJ_LJP(1, 1, 3),
	/* EG_LJ422 */ MIJ_LJP(2, 1, 3),
	/* EG_LJ420 */ MIJ_LJP(2, 2, 3),
	/* EG_LJGREY */ MIJ_LJP(1, 1, 1),
};
#undef MIJ_ENCP
#undef MIJ_LJC
#undef MIJ_LJP

struct EncSlot {
	mjw_tplan tp; /* the slot's plan, whatever its kind: a pixel slot without options has the writer's 4:2:0 or 4:4:4 */
	EncImage dev;
	size_t stage_off, pix_bytes, du_bytes;
	int pad_w; /* pixels per staged row: the width rounded up to whole MCU columns (enc_padded_width); staged rows are packed RGB */
	int clone_of, flip;
	EncKind kind;               /* a clone copies its root's pixels whatever the root's kind */
	bool optimize;              /* mij_enc_set_optimize */
	int restart;                /* mij_enc_set_restart: the restart interval in MCUs, 0: none */
	bool progressive;           /* mij_enc_set_progressive */
	int arith;                  /* mij_enc_set_arith: MIJ_ARITH_STB, or MIJ_ARITH_LIBJPEG (include/mij_host.h, LIBJPEG ENCODING) */
	mij_in_tensor in;           /* ENC_DEVICE */
	mij_in_convert cv;          /* ENC_DEVICE with float elements (mij_enc_add_device_float); cv.dtype is MIJ_DT_U8 for every other slot */
	std::vector<int16_t> units; /* ENC_UNITS */
	/* ENC_COEF (mij_enc_add_coef): the batch, and where the slot's planes lay when it was added */
	mij_batch *src;
	CoefSlot coef;
	int coef_fmt;
	int rect[4];                  /* the kept rectangle in the displayed frame (mij_enc_slot_rect) */
	bool greyed;                  /* Cb and Cr of a colour source were dropped */
	bool sampled;                 /* a pixel slot made with a sampling or tables of its own (mij_enc_add_ex and its kin): mij_enc_tplan answers */
	bool planes;                  /* a plane slot (mij_enc_add_planes, mij_enc_add_device_planes): sampled too; the staging is planar */
	mij_plane pl[3];              /* its planes, ENC_DEVICE only */
	bool pl_convert;              /* cv holds its range conversion (dtype MIJ_DT_U8; entries 0..2: Y, Cb, Cr) */
	unsigned char rq_from[2][64]; /* a requantising slot (coef.rq != 0): the tables tp's replaced, luma and chroma, zigzag order */
};

/* GPU emission (mij_enc_stream_reserve): everything enc_free_emit gives back */
struct EncEmit {
	Buf<uint8_t> arena; /* the streams, and the pinned mirror mij_enc_stream points into; bytes */
	/* the code tables: entry 0 the plain ones (h_tabs0), entry k + 1 those of the k-th optimised slot, then MIJ_PROG_SCANS per progressive slot */
	Buf<EmitTables, BUF_ON_DEVICE> tabs;
	EmitTables h_tabs0;
	/* per-slot and per-tile lists, the headers (MIJ_EMIT_HDR bytes each), the results */
	Buf<EmitSlot> eslot;
	Buf<EmitTile> etile;
	Buf<uint8_t> hdr;
	Buf<EmitResult> res;
	Buf<uint32_t, BUF_ON_DEVICE> tbits, tff, tfrag;
	Buf<uint64_t, BUF_ON_DEVICE> tboff, tout, sent;
	size_t n_etile = 0;
	/* optimised Huffman tables (mij_enc_set_optimize): the optimised slots' tiles, their slot numbers, their counts and whether each kept
	 * its own tables */
	Buf<EmitTile> otile;
	Buf<uint32_t> optslot;
	Buf<uint32_t, BUF_ON_DEVICE> freq, optok;
	size_t n_otile = 0, n_opt = 0;
	/* progressive slots (mij_enc_set_progressive; mij_progressive_kernels.h): their records, the numbers of their tiles in the tile list, the
	 * block bytes of their AC scans, scan headers and their lengths, per-tile summaries and run results, per-scan counts, and the per-slot
	 * flag of the slots the host finishes (a forced flush, a table that cannot be built) */
	Buf<ProgSlot> pslot;
	Buf<uint32_t> ptile;
	Buf<uint8_t, BUF_ON_DEVICE> pfl, phdr;
	Buf<ProgTileSum, BUF_ON_DEVICE> tsum;
	Buf<ProgAfter, BUF_ON_DEVICE> tafter;
	Buf<uint32_t, BUF_ON_DEVICE> pfreq, phlen, pflag, ctail;
	size_t n_prog = 0, n_ptile = 0;
};

struct mij_encoder {
	mij_ctx *ctx = nullptr;
	hipStream_t stream = nullptr;
	hipEvent_t ev_begin = nullptr, ev_end = nullptr;
	int max_images = 0;
	/* the arenas, sized at creation, in bytes: pinned pixels, device pixels, the data units and their pinned mirror (made at the first
	 * mij_enc_fetch_all) */
	Buf<uint8_t, BUF_PINNED> stage;
	Buf<uint8_t, BUF_ON_DEVICE> pix;
	Buf<uint8_t, BUF_ON_DEVICE> du;
	Buf<uint8_t, BUF_PINNED> du_host;
	size_t stage_used = 0, pix_used = 0, du_used = 0;
	Buf<EncImage> imgs; /* max_images of them */
	Buf<WorkIdct> work;  /* the transform kernels' work items, group after group */
	size_t n_work[EG_GROUPS] = {}, first_work[EG_GROUPS] = {};
	std::vector<EncSlot> slots;
	bool uploaded = false, launched = false, force_generic = false;
	/* device-pixel slots: the gather kernels' slots and work (rows of MIJ_GATHER_ROWS) for uint8 tensors, float tensors (grouped by dtype:
	 * one launch of k_enc_gather_float each) and planes (k_enc_gather_planes) */
	Buf<EncGather> gath;
	Buf<EncGatherF> fgath;
	Buf<EncGatherP> pgath;
	Buf<WorkIdct> gwork, fgwork, pgwork;
	/* libjpeg slots (mij_enc_set_arith): one LjEncSlot per slot and the planes pass 1 leaves for pass 2, both grown at upload */
	Buf<LjEncSlot> lj;
	Buf<uint8_t, BUF_ON_DEVICE> lj_planes;
	EncEmit em;
	bool emit_queued = false, streams_fetched = false;
	std::vector<int> opt_of;      /* slot -> k, or -1 */
	std::vector<uint32_t> opt_ok; /* after mij_enc_fetch_streams */
	std::vector<uint32_t> pflag;  /* after mij_enc_fetch_streams */
	/* coefficient slots (mij_enc_add_coef): the conversion kernel's slots and work (plane tiles), one table per requantising slot of the
	 * upload (CoefSlot::rq - 1), the event that orders it behind the batch's stream, and the per-slot flags it raises for uncodable
	 * values (sflag_dev: one per slot, read by k_emit_count) */
	Buf<CoefSlot> cslot;
	Buf<WorkIdct> cwork;
	Buf<RqTable> rqt;
	Buf<uint32_t, BUF_ON_DEVICE> sflag_dev;
	hipEvent_t ev_coef = nullptr;
	bool has_coef = false;       /* the last upload had a coefficient slot */
	uint32_t coef_tiles = 0;     /* plane tiles its conversion queued (mij_enc_coef_tiles) */
	std::vector<uint32_t> sflag; /* after mij_enc_fetch_streams */
	hipEvent_t ev_conv0 = nullptr, ev_conv1 = nullptr; /* around the conversion kernels of the last upload (mij_enc_coef_ms) */
	bool conv_timed = false;
};

static void enc_free_emit(mij_encoder *e)
{
	e->em = EncEmit();
	e->emit_queued = e->streams_fetched = false;
}

extern "C" int mij_enc_create(mij_ctx *ctx, int max_images, size_t pixel_bytes, size_t du_bytes, mij_encoder **out)
{
	return mij_enc_create_ex(ctx, max_images, pixel_bytes, pixel_bytes, du_bytes, out);
}

extern "C" int mij_enc_create_ex(mij_ctx *ctx, int max_images, size_t stage_bytes, size_t pixel_bytes, size_t du_bytes, mij_encoder **out)
{
	if (!ctx || !out || max_images <= 0)
		return set_err(MIJ_E_ARG, "mij_enc_create: bad argument");
	*out = nullptr;
	HIP_TRY(hipSetDevice(ctx->device));
	mij_encoder *e = new (std::nothrow) mij_encoder();
	if (!e)
		return set_err(MIJ_E_NOMEM, "out of host memory");
	e->ctx = ctx;
	e->max_images = max_images;
	e->force_generic = getenv("MIJ_ENC_GENERIC") != nullptr;
	hipError_t r = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
	if (r == hipSuccess)
		r = hipEventCreate(&e->ev_begin);
	if (r == hipSuccess)
		r = hipEventCreate(&e->ev_end);
	if (r == hipSuccess)
		r = e->stage.alloc(stage_bytes);
	if (r == hipSuccess)
		r = e->pix.alloc(pixel_bytes);
	if (r == hipSuccess)
		r = e->du.alloc(du_bytes);
	if (r == hipSuccess)
		r = e->imgs.alloc((size_t)max_images);
	if (r != hipSuccess) {
		int code = (r == hipErrorOutOfMemory) ? MIJ_E_NOMEM : MIJ_E_HIP;
		set_err(code, "mij_enc_create: %s", hipGetErrorString(r));
		mij_enc_destroy(e);
		return code;
	}
	*out = e;
	return MIJ_OK;
}

extern "C" void mij_enc_destroy(mij_encoder *e)
{
	if (!e)
		return;
	(void)hipSetDevice(e->ctx->device);
	if (e->stream)
		(void)hipStreamSynchronize(e->stream);
	const hipStream_t stream = e->stream;
	const hipEvent_t events[] = {e->ev_coef, e->ev_conv0, e->ev_conv1, e->ev_begin, e->ev_end};
	delete e; /* its buffers release themselves, before the events and the stream go */
	for (hipEvent_t ev : events)
		if (ev)
			(void)hipEventDestroy(ev);
	if (stream)
		(void)hipStreamDestroy(stream);
}

extern "C" int mij_enc_reset(mij_encoder *e)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	HIP_TRY(hipSetDevice(e->ctx->device));
	HIP_TRY(hipStreamSynchronize(e->stream));
	e->slots.clear();
	e->stage_used = e->pix_used = e->du_used = 0;
	e->uploaded = e->launched = false;
	e->emit_queued = e->streams_fetched = false;
	return MIJ_OK;
}

/* Every picture is staged as packed RGB with rows of whole MCU columns: the last pixel of a row repeated into the padding -- the reference's
 * edge rule (codec/jpeg_write.c:294-296) applied once on the way in -- and, round 3, the reference's channel rule applied there too
 * (codec/jpeg_write.c:276-279: "ofsG = comp > 2 ? 1 : 0, ofsB = comp > 2 ? 2 : 0", r = data[p]): a grey or grey + alpha picture becomes
 * r = g = b = grey, an RGBA picture loses its alpha.  The device therefore only ever sees three channels, the same float expressions run on the
 * same values, and the strip kernels (k_encode420 / k_encode444: 16-byte or 8-byte row chunks, no column clamp) take every width and every
 * `comp`, not only RGB at multiples of 16 / 8 (the per-unit kernels remain as their test twins, mij_enc_force_generic). */
static int enc_padded_width(int width, int lh)
{
	const int unit = 8 * lh; /* the MCU width of the slot's sampling */
	return (width + unit - 1) / unit * unit;
}
static void enc_stage_rows(uint8_t *dst, const uint8_t *src, int width, int height, int comp, int pad_w)
{
	if (comp == 3 && pad_w == width) {
		memcpy(dst, src, (size_t)width * height * 3);
		return;
	}
	const size_t in_pitch = (size_t)width * comp, out_pitch = (size_t)pad_w * 3;
	const int og = comp > 2 ? 1 : 0, ob = comp > 2 ? 2 : 0;
	for (int y = 0; y < height; ++y) {
		uint8_t *d = dst + (size_t)y * out_pitch;
		const uint8_t *p = src + (size_t)y * in_pitch;
		if (comp == 3)
			memcpy(d, p, in_pitch);
		else
			for (int x = 0; x < width; ++x) {
				d[3 * x] = p[(size_t)x * comp];
				d[3 * x + 1] = p[(size_t)x * comp + og];
				d[3 * x + 2] = p[(size_t)x * comp + ob];
			}
		for (int x = width; x < pad_w; ++x)
			memcpy(d + (size_t)x * 3, d + (size_t)(width - 1) * 3, 3);
	}
}
/* the plan of a pixel slot under its options (NULL or all zero: as the writer itself chooses) */
static int enc_opts_plan(mjw_tplan *t, int width, int height, int comp, int quality, const mij_enc_opts *o)
{
	return mjw_splan_init(t, width, height, comp, quality, o ? o->ncomp : 0, o ? o->lh : 0, o ? o->lv : 0, o ? o->luma : nullptr, o ? o->chroma : nullptr);
}
static bool enc_opts_given(const mij_enc_opts *o) { return o && (o->ncomp || o->lh || o->lv || o->luma || o->chroma); }

extern "C" size_t mij_enc_pixel_bytes_ex(int width, int height, int comp, int quality, const mij_enc_opts *opts)
{
	mjw_tplan t;
	if (!enc_opts_plan(&t, width, height, comp, quality, opts))
		return 0;
	return align_up((size_t)enc_padded_width(width, t.lh) * height * 3, 256);
}
extern "C" size_t mij_enc_pixel_bytes(int width, int height, int comp, int quality) { return mij_enc_pixel_bytes_ex(width, height, comp, quality, nullptr); }

/* a plane slot's share of the pixel arenas: luma blocks plus two chroma blocks per MCU, 64 samples each */
static size_t enc_plane_bytes(const mjw_tplan &t)
{
	return align_up((size_t)t.plan.mcu_x * (size_t)t.plan.mcu_y * (size_t)t.plan.du_per_mcu * 64, 256);
}
extern "C" size_t mij_enc_plane_bytes(int width, int height, const mij_enc_opts *opts)
{
	mjw_tplan t;
	if (!opts || !mjw_pplan_init(&t, width, height, 0, opts->ncomp, opts->lh, opts->lv, nullptr, nullptr))
		return 0;
	return enc_plane_bytes(t);
}

static int enc_add_common(mij_encoder *e, const mjw_tplan &tplan, const void *pixels, int flip, int clone_of, EncKind kind = ENC_HOST, bool sampled = false,
                          bool planes = false)
{
	const mjw_plan &plan = tplan.plan;
	if ((int)e->slots.size() >= e->max_images)
		return set_err(MIJ_E_NOMEM, "encoder batch is full (%d images)", e->max_images);
	EncSlot s;
	s.tp = tplan;
	s.flip = flip;
	s.clone_of = clone_of;
	s.kind = kind;
	s.optimize = false;
	s.progressive = false;
	s.restart = 0;
	s.arith = MIJ_ARITH_STB;
	memset(&s.in, 0, sizeof(s.in));
	memset(&s.cv, 0, sizeof(s.cv));
	s.cv.dtype = MIJ_DT_U8;
	s.pad_w = enc_padded_width(plan.width, tplan.ncomp == 1 ? 1 : tplan.lh);
	s.src = nullptr;
	s.coef_fmt = 0;
	s.sampled = sampled;
	s.planes = planes;
	memset(s.pl, 0, sizeof(s.pl));
	s.pl_convert = false;
	memset(&s.coef, 0, sizeof(s.coef));
	memset(s.rq_from, 0, sizeof(s.rq_from));
	memset(s.rect, 0, sizeof(s.rect));
	s.greyed = false;
	s.pix_bytes = !enc_has_pixels(kind) ? 0 : align_up((size_t)s.pad_w * plan.height * 3, 256); /* staged as packed RGB whatever plan.comp is (enc_stage_rows) */
	if (planes) /* planar, every plane padded to whole MCUs of its component both ways */
		s.pix_bytes = enc_plane_bytes(tplan);
	s.du_bytes = align_up(mjw_plan_du_count(&plan) * 128, 256);
	if (e->pix_used + s.pix_bytes > e->pix.cap)
		return set_err(MIJ_E_NOMEM, "pixel arena exhausted");
	if (e->du_used + s.du_bytes > e->du.cap)
		return set_err(MIJ_E_NOMEM, "data-unit arena exhausted");
	if (clone_of < 0 && kind != ENC_HOST) {
		s.stage_off = 0; /* no pinned staging: the gather kernel or the units' own copy fills the device side */
	} else if (clone_of < 0) {
		if (e->stage_used + s.pix_bytes > e->stage.cap)
			return set_err(MIJ_E_NOMEM, "pixel staging exhausted");
		s.stage_off = e->stage_used;
		if (pixels) /* mij_enc_add_uncopied: the caller stages the pixels itself (mij_enc_stage_pixels, several threads at once) */
			enc_stage_rows(e->stage.h + s.stage_off, static_cast<const uint8_t *>(pixels), plan.width, plan.height, plan.comp, s.pad_w);
		e->stage_used += s.pix_bytes;
	} else {
		s.stage_off = e->slots[(size_t)clone_of].stage_off;
	}
	memset(&s.dev, 0, sizeof(s.dev));
	s.dev.width = s.pad_w; /* the device sees whole MCU columns */
	s.dev.height = plan.height;
	s.dev.comp = 3; /* what the staging holds */
	s.dev.subsample = plan.subsample;
	s.dev.mcu_x = plan.mcu_x;
	s.dev.mcu_y = plan.mcu_y;
	s.dev.flip = flip;
	if (planes) { /* k_encode_planes derives the staged geometry from mcu_x and mcu_y */
		s.dev.height = plan.mcu_y * 8 * tplan.lv;
		s.dev.comp = 1;
		s.dev.flip = 0; /* applied on the way into the staging */
	}
	s.dev.pix_off = e->pix_used;
	s.dev.du_off = e->du_used;
	memcpy(s.dev.fy, plan.fdtbl_y, sizeof(s.dev.fy));
	memcpy(s.dev.fc, plan.fdtbl_c, sizeof(s.dev.fc));
	e->pix_used += s.pix_bytes;
	e->du_used += s.du_bytes;
	e->slots.push_back(std::move(s));
	e->uploaded = e->launched = false;
	e->emit_queued = e->streams_fetched = false;
	return (int)e->slots.size() - 1;
}

extern "C" int mij_enc_add_ex(mij_encoder *e, const void *pixels, int width, int height, int comp, int quality, int flip_vertically,
                              const mij_enc_opts *opts)
{
	if (!e || !pixels)
		return set_err(MIJ_E_ARG, "bad argument");
	mjw_tplan t;
	if (!enc_opts_plan(&t, width, height, comp, quality, opts))
		return set_err(MIJ_E_ARG, "bad image arguments (%dx%dx%d), sampling or tables", width, height, comp);
	return enc_add_common(e, t, pixels, flip_vertically ? 1 : 0, -1, ENC_HOST, enc_opts_given(opts));
}
extern "C" int mij_enc_add(mij_encoder *e, const void *pixels, int width, int height, int comp, int quality, int flip_vertically)
{
	return mij_enc_add_ex(e, pixels, width, height, comp, quality, flip_vertically, nullptr);
}

extern "C" int mij_enc_add_uncopied_ex(mij_encoder *e, int width, int height, int comp, int quality, int flip_vertically, const mij_enc_opts *opts)
{
	if (!e)
		return set_err(MIJ_E_ARG, "bad argument");
	mjw_tplan t;
	if (!enc_opts_plan(&t, width, height, comp, quality, opts))
		return set_err(MIJ_E_ARG, "bad image arguments (%dx%dx%d), sampling or tables", width, height, comp);
	return enc_add_common(e, t, nullptr, flip_vertically ? 1 : 0, -1, ENC_HOST, enc_opts_given(opts));
}
extern "C" int mij_enc_add_uncopied(mij_encoder *e, int width, int height, int comp, int quality, int flip_vertically)
{
	return mij_enc_add_uncopied_ex(e, width, height, comp, quality, flip_vertically, nullptr);
}

extern "C" int mij_enc_stage_pixels(mij_encoder *e, int slot, const void *pixels)
{
	if (!e || !pixels || slot < 0 || slot >= (int)e->slots.size() || e->slots[(size_t)slot].clone_of >= 0 || e->slots[(size_t)slot].kind != ENC_HOST ||
		 e->slots[(size_t)slot].planes)
		return set_err(MIJ_E_ARG, "bad slot or pixels");
	const EncSlot &s = e->slots[(size_t)slot];
	enc_stage_rows(e->stage.h + s.stage_off, static_cast<const uint8_t *>(pixels), s.tp.plan.width, s.tp.plan.height, s.tp.plan.comp, s.pad_w);
	return MIJ_OK;
}

extern "C" void *mij_enc_staging(mij_encoder *e, int slot)
{
	if (!e || slot < 0 || slot >= (int)e->slots.size() || e->slots[(size_t)slot].clone_of >= 0 || e->slots[(size_t)slot].kind != ENC_HOST)
		return nullptr;
	return e->stage.h + e->slots[(size_t)slot].stage_off;
}

/* every slot's data units into the encoder's pinned mirror in one copy; mij_enc_units(slot) then points at a slot's units */
extern "C" int mij_enc_fetch_all(mij_encoder *e)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	if (!e->launched)
		return set_err(MIJ_E_STATE, "mij_enc_fetch_all before launch");
	HIP_TRY(hipSetDevice(e->ctx->device));
	if (!e->du_host.h)
		HIP_TRY(e->du_host.alloc(e->du.cap));
	if (e->du_used)
		HIP_TRY(hipMemcpyAsync(e->du_host.h, e->du.d, e->du_used, hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return MIJ_OK;
}

/* the same without the wait: mij_enc_wait before mij_enc_units is read */
extern "C" int mij_enc_fetch_all_async(mij_encoder *e)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	if (!e->launched)
		return set_err(MIJ_E_STATE, "mij_enc_fetch_all_async before launch");
	HIP_TRY(hipSetDevice(e->ctx->device));
	if (!e->du_host.h)
		HIP_TRY(e->du_host.alloc(e->du.cap));
	if (e->du_used)
		HIP_TRY(hipMemcpyAsync(e->du_host.h, e->du.d, e->du_used, hipMemcpyDeviceToHost, e->stream));
	return MIJ_OK;
}

extern "C" const int16_t *mij_enc_units(const mij_encoder *e, int slot)
{
	if (!e || !e->du_host.h || slot < 0 || slot >= (int)e->slots.size())
		return nullptr;
	return reinterpret_cast<const int16_t *>(e->du_host.h + e->slots[(size_t)slot].dev.du_off);
}

/* the slot, or NULL with MIJ_E_ARG and `what` as the error */
static const EncSlot *enc_slot(const mij_encoder *e, int slot, const char *what = "bad slot")
{
	if (!e || slot < 0 || slot >= (int)e->slots.size()) {
		set_err(MIJ_E_ARG, "%s", what);
		return nullptr;
	}
	return &e->slots[(size_t)slot];
}
static EncSlot *enc_slot(mij_encoder *e, int slot, const char *what = "bad slot")
{
	return const_cast<EncSlot *>(enc_slot(static_cast<const mij_encoder *>(e), slot, what));
}

extern "C" int mij_enc_add_clone(mij_encoder *e, int src_slot)
{
	const EncSlot *src = enc_slot(e, src_slot, "bad source slot");
	if (!src)
		return MIJ_E_ARG;
	const int root = src->clone_of >= 0 ? src->clone_of : src_slot;
	const EncSlot &r = e->slots[(size_t)root];
	if (!enc_has_pixels(r.kind))
		return set_err(MIJ_E_ARG, "slot %d holds given data units or coefficient planes, which have no pixels to clone", src_slot);
	const bool optimize = src->optimize, progressive = src->progressive; /* src and r do not outlive the push */
	const int restart = src->restart, arith = src->arith;
	const int slot = enc_add_common(e, mjw_tplan(r.tp), nullptr, r.flip, root, ENC_HOST, r.sampled, r.planes);
	if (slot >= 0) {
		e->slots[(size_t)slot].optimize = optimize;
		e->slots[(size_t)slot].restart = restart;
		e->slots[(size_t)slot].progressive = progressive;
		e->slots[(size_t)slot].arith = arith;
	}
	return slot;
}

/* natural index (8 * row + column) -> zigzag position, the order quantisation tables are kept in */
static const uint8_t enc_zigzag_of[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
														10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

/* include/mij.h: libjpeg's arithmetic and header for a pixel or plane slot (include/mij_host.h, LIBJPEG ENCODING) */
extern "C" int mij_enc_set_arith(mij_encoder *e, int slot, int arith)
{
	EncSlot *s = enc_slot(e, slot);
	if (!s)
		return MIJ_E_ARG;
	if (arith != MIJ_ARITH_STB && arith != MIJ_ARITH_LIBJPEG)
		return set_err(MIJ_E_ARG, "mij_enc_set_arith: arithmetic %d is neither MIJ_ARITH_STB nor MIJ_ARITH_LIBJPEG", arith);
	if (e->uploaded)
		return set_err(MIJ_E_STATE, "mij_enc_set_arith after mij_enc_upload");
	if (arith == MIJ_ARITH_LIBJPEG) {
		if (!enc_has_pixels(s->kind))
			return set_err(MIJ_E_ARG, "slot %d holds given data units or coefficient planes: there is nothing to transform", slot);
		if (s->tp.ncomp == 3 && s->tp.lh == 1 && s->tp.lv == 2)
			return set_err(MIJ_E_ARG, "slot %d is 4:4:0, which libjpeg's arithmetic does not serve (no writer to judge it)", slot);
		if (s->tp.plan.comp != 1 && s->tp.plan.comp != 3)
			return set_err(MIJ_E_ARG, "slot %d has %d channels: libjpeg's arithmetic serves 1 and 3", slot, s->tp.plan.comp);
	}
	s->arith = arith;
	return MIJ_OK;
}

extern "C" int mij_enc_group_work(const mij_encoder *e, int group)
{
	if (!e || group < 0 || group >= EG_GROUPS)
		return set_err(MIJ_E_ARG, "bad encoder or group");
	if (!e->uploaded)
		return set_err(MIJ_E_STATE, "mij_enc_group_work before mij_enc_upload");
	return (int)e->n_work[group];
}

extern "C" int mij_enc_slot_arith(const mij_encoder *e, int slot)
{
	const EncSlot *s = enc_slot(e, slot);
	return s ? s->arith : MIJ_E_ARG;
}

extern "C" int mij_enc_set_optimize(mij_encoder *e, int slot, int on)
{
	EncSlot *s = enc_slot(e, slot);
	if (!s)
		return MIJ_E_ARG;
	if (e->uploaded)
		return set_err(MIJ_E_STATE, "mij_enc_set_optimize after mij_enc_upload");
	if (on && mjw_plan_du_count(&s->tp.plan) > (size_t)(UINT32_MAX / 64))
		return set_err(MIJ_E_ARG, "slot %d: the symbol counts of %zu data units do not fit 32 bits", slot, mjw_plan_du_count(&s->tp.plan));
	s->optimize = on != 0;
	return MIJ_OK;
}

extern "C" int mij_enc_set_restart(mij_encoder *e, int slot, int restart_mcus)
{
	EncSlot *s = enc_slot(e, slot);
	if (!s)
		return MIJ_E_ARG;
	if (e->uploaded)
		return set_err(MIJ_E_STATE, "mij_enc_set_restart after mij_enc_upload");
	if (restart_mcus < 0 || restart_mcus > 65535)
		return set_err(MIJ_E_ARG, "slot %d: a restart interval of %d MCUs is outside 0..65535", slot, restart_mcus);
	if (restart_mcus && s->progressive)
		return set_err(MIJ_E_ARG, "slot %d is progressive: restart intervals are not combined with progressive output", slot);
	/* given units were judged unbroken when they were added: with an interval the DC differences are other ones */
	const char *why = nullptr;
	if (s->kind == ENC_UNITS && restart_mcus && !mjw_units_codable_restart(&s->tp.plan, s->units.data(), restart_mcus, &why))
		return set_err(MIJ_E_ARG, "slot %d at a restart interval of %d MCUs: %s", slot, restart_mcus, why ? why : "not codable");
	s->restart = restart_mcus;
	return MIJ_OK;
}

extern "C" int mij_enc_set_progressive(mij_encoder *e, int slot, int on)
{
	EncSlot *s = enc_slot(e, slot);
	if (!s)
		return MIJ_E_ARG;
	if (e->uploaded)
		return set_err(MIJ_E_STATE, "mij_enc_set_progressive after mij_enc_upload");
	if (on && s->restart)
		return set_err(MIJ_E_ARG, "slot %d has a restart interval: restart intervals are not combined with progressive output", slot);
	if (on && mjw_plan_du_count(&s->tp.plan) > (size_t)(UINT32_MAX / 64))
		return set_err(MIJ_E_ARG, "slot %d: the symbol counts of %zu data units do not fit 32 bits", slot, mjw_plan_du_count(&s->tp.plan));
	s->progressive = on != 0;
	return MIJ_OK;
}

extern "C" int mij_enc_slot_progressive(const mij_encoder *e, int slot)
{
	const EncSlot *s = enc_slot(e, slot);
	return s ? (s->progressive ? 1 : 0) : MIJ_E_ARG;
}

extern "C" int mij_enc_slot_restart(const mij_encoder *e, int slot)
{
	const EncSlot *s = enc_slot(e, slot);
	return s ? s->restart : MIJ_E_ARG;
}

extern "C" int mij_enc_slot_optimized(const mij_encoder *e, int slot)
{
	if (!enc_slot(e, slot))
		return MIJ_E_ARG;
	if (!e->streams_fetched)
		return set_err(MIJ_E_STATE, "mij_enc_slot_optimized before mij_enc_fetch_streams");
	const int k = e->opt_of[(size_t)slot];
	return k >= 0 && e->opt_ok[(size_t)k] ? 1 : 0;
}

/* One gather pass, queued at upload in place of a host-to-device copy.  The device slots that takes(slot, k) names get a record each in
 * `list` (fill) and their work items in `work` (items(slot, push) calls push(component, first row) for each, in order), class k = 0 ..
 * CLASSES - 1 after class; launch(k, work, grid) then runs once per class that has work.  Nothing is queued when there are no such slots. */
template <int CLASSES, typename G, typename Takes, typename Items, typename Fill, typename Launch>
static int enc_gather_pass(mij_encoder *e, Buf<G> &list, Buf<WorkIdct> &work, Takes takes, Items items, Fill fill, Launch launch)
{
	const auto gathered = [&](const EncSlot &s, int k) { return s.clone_of < 0 && s.kind == ENC_DEVICE && takes(s, k); };
	size_t ng = 0, nw = 0;
	for (int k = 0; k < CLASSES; ++k)
		for (const EncSlot &s : e->slots)
			if (gathered(s, k)) {
				++ng;
				items(s, [&](uint32_t, uint32_t) { ++nw; });
			}
	if (!ng)
		return MIJ_OK;
	Grow grow(e->stream);
	grow(list, ng);
	grow(work, nw);
	if (grow.rc != MIJ_OK)
		return grow.rc;
	size_t first[CLASSES + 1] = {0};
	uint32_t g = 0;
	size_t w = 0;
	for (int k = 0; k < CLASSES; ++k) {
		for (const EncSlot &s : e->slots) {
			if (!gathered(s, k))
				continue;
			fill(list.h[g], s);
			items(s, [&](uint32_t c, uint32_t y) { work.h[w++] = WorkIdct{g, c, y, 0u}; });
			++g;
		}
		first[k + 1] = w;
	}
	HIP_TRY(hipMemcpyAsync(list.d, list.h, sizeof(G) * ng, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(work.d, work.h, sizeof(WorkIdct) * nw, hipMemcpyHostToDevice, e->stream));
	for (int k = 0; k < CLASSES; ++k) {
		if (first[k + 1] == first[k])
			continue;
		launch(k, work.d + first[k], dim3((unsigned)(first[k + 1] - first[k])));
		HIP_TRY(hipGetLastError());
	}
	return MIJ_OK;
}

/* a device tensor's record and its work items: the padded packed-RGB rows, MIJ_GATHER_ROWS at a time */
static void enc_gather_fill(EncGather &G, const EncSlot &s)
{
	G.src = static_cast<const uint8_t *>(s.in.src);
	G.row_pitch = s.in.row_pitch;
	G.plane_pitch = s.in.plane_pitch;
	G.layout = s.in.layout;
	G.width = s.tp.plan.width;
	G.height = s.tp.plan.height;
	G.comp = s.tp.plan.comp;
	G.pad_w = s.pad_w;
	G.pad = 0;
	G.pix_off = s.dev.pix_off;
}
template <typename Push>
static void enc_gather_rows(const EncSlot &s, Push push)
{
	for (uint32_t y = 0; y < (uint32_t)s.tp.plan.height; y += MIJ_GATHER_ROWS)
		push(0u, y);
}

/* the uint8 device-pixel slots (mij_enc_add_device): k_enc_gather */
static int enc_gather(mij_encoder *e)
{
	return enc_gather_pass<1>(
		e, e->gath, e->gwork, [](const EncSlot &s, int) { return s.cv.dtype == MIJ_DT_U8 && !s.planes; },
		[](const EncSlot &s, auto push) { enc_gather_rows(s, push); }, enc_gather_fill,
		[e](int, const WorkIdct *wk, dim3 grid) { hipLaunchKernelGGL(k_enc_gather, grid, dim3(256), 0, e->stream, e->gath.d, wk, e->pix.d); });
}

/* the float ones (mij_enc_add_device_float), grouped by dtype: one launch of k_enc_gather_float per dtype that has slots */
static int enc_gather_float(mij_encoder *e)
{
	static const int32_t dts[3] = {MIJ_DT_F16, MIJ_DT_BF16, MIJ_DT_F32};
	return enc_gather_pass<3>(
		e, e->fgath, e->fgwork, [](const EncSlot &s, int k) { return s.cv.dtype == dts[k] && !s.planes; },
		[](const EncSlot &s, auto push) { enc_gather_rows(s, push); },
		[](EncGatherF &G, const EncSlot &s) {
			enc_gather_fill(G.g, s);
			memcpy(G.scale, s.cv.scale, sizeof(G.scale));
			memcpy(G.bias, s.cv.bias, sizeof(G.bias));
		},
		[e](int k, const WorkIdct *wk, dim3 grid) {
			const auto kernel = dts[k] == MIJ_DT_F16 ? k_enc_gather_float<GatherF16> : dts[k] == MIJ_DT_BF16 ? k_enc_gather_float<GatherBF16> : k_enc_gather_float<GatherF32>;
			hipLaunchKernelGGL(kernel, grid, dim3(256), 0, e->stream, e->fgath.d, wk, e->pix.d);
		});
}

/* the device plane slots (mij_enc_add_device_planes): k_enc_gather_planes, rows of MIJ_PGATHER_ROWS of each padded plane */
static void enc_plane_geometry(const mjw_tplan &t, int c, int32_t *w, int32_t *h, int32_t *pad_w, int32_t *pad_h)
{
	const int lh = c ? 1 : t.lh, lv = c ? 1 : t.lv;
	*w = c ? (t.plan.width + t.lh - 1) / t.lh : t.plan.width;
	*h = c ? (t.plan.height + t.lv - 1) / t.lv : t.plan.height;
	*pad_w = t.plan.mcu_x * 8 * lh;
	*pad_h = t.plan.mcu_y * 8 * lv;
}

static int enc_gather_planes(mij_encoder *e)
{
	return enc_gather_pass<1>(
		e, e->pgath, e->pgwork, [](const EncSlot &s, int) { return s.planes; },
		[](const EncSlot &s, auto push) {
			for (int c = 0; c < s.tp.ncomp; ++c) {
				int32_t w, h, pad_w, pad_h;
				enc_plane_geometry(s.tp, c, &w, &h, &pad_w, &pad_h);
				for (uint32_t y = 0; y < (uint32_t)pad_h; y += MIJ_PGATHER_ROWS)
					push((uint32_t)c, y);
			}
		},
		[](EncGatherP &G, const EncSlot &s) {
			memset(&G, 0, sizeof(G));
			uint64_t off = s.dev.pix_off;
			for (int c = 0; c < s.tp.ncomp; ++c) {
				G.src[c] = static_cast<const uint8_t *>(s.pl[c].src);
				G.row_pitch[c] = s.pl[c].row_pitch;
				G.x_pitch[c] = s.pl[c].x_pitch;
				enc_plane_geometry(s.tp, c, &G.w[c], &G.h[c], &G.pad_w[c], &G.pad_h[c]);
				G.dst_off[c] = off;
				off += (uint64_t)G.pad_w[c] * (uint64_t)G.pad_h[c];
				G.scale[c] = s.cv.scale[c];
				G.bias[c] = s.cv.bias[c];
			}
			G.flip = s.flip;
			G.convert = s.pl_convert ? 1 : 0;
		},
		[e](int, const WorkIdct *wk, dim3 grid) { hipLaunchKernelGGL(k_enc_gather_planes, grid, dim3(256), 0, e->stream, e->pgath.d, wk, e->pix.d); });
}

/* a host plane slot's staging: the layout k_enc_gather_planes makes, by the same rules */
static void enc_stage_planes(uint8_t *dst, const mjw_tplan &t, const mij_plane *pl, const mij_in_convert *cv, int flip)
{
	for (int c = 0; c < t.ncomp; ++c) {
		int32_t w, h, pad_w, pad_h;
		enc_plane_geometry(t, c, &w, &h, &pad_w, &pad_h);
		uint8_t lut[256];
		for (int i = 0; i < 256; ++i) {
			float v = (float)i;
			if (cv) {
				v = v * cv->scale[c];
				v = v + cv->bias[c];
				v = rintf(fminf(fmaxf(v, 0.0f), 255.0f));
			}
			lut[i] = (uint8_t)v;
		}
		const uint8_t *src = static_cast<const uint8_t *>(pl[c].src);
		for (int y = 0; y < pad_h; ++y) {
			const int cy = y < h ? y : h - 1;
			const uint8_t *row = src + (int64_t)(flip ? h - 1 - cy : cy) * pl[c].row_pitch;
			uint8_t *d = dst + (size_t)y * (size_t)pad_w;
			for (int x = 0; x < w; ++x)
				d[x] = lut[row[(int64_t)x * pl[c].x_pitch]];
			memset(d + w, d[w - 1], (size_t)(pad_w - w));
		}
		dst += (size_t)pad_w * (size_t)pad_h;
	}
}

static int enc_add_planes(mij_encoder *e, const mij_in_planes *p, int quality, bool device)
{
	if (!e || !p)
		return set_err(MIJ_E_ARG, "bad argument");
	mjw_tplan t;
	if (!mjw_pplan_init(&t, p->width, p->height, quality, p->opts.ncomp, p->opts.lh, p->opts.lv, p->opts.luma, p->opts.chroma))
		return set_err(MIJ_E_ARG, "bad plane arguments (%dx%d): the sampling (%d, %d, %d) is required and one of the five, tables come in pairs of entries 1..255",
							p->width, p->height, p->opts.ncomp, p->opts.lh, p->opts.lv);
	const mij_in_convert *cv = p->convert;
	if (cv && cv->dtype != MIJ_DT_U8)
		return set_err(MIJ_E_ARG, "planes hold uint8 samples: convert->dtype must be MIJ_DT_U8");
	const int64_t lim = (int64_t)1 << 40;
	for (int c = 0; c < 3; ++c) {
		const mij_plane &q = p->planes[c];
		if (c >= t.ncomp) {
			if (q.src)
				return set_err(MIJ_E_ARG, "a grey slot takes no chroma plane (planes[%d].src is not NULL)", c);
			continue;
		}
		int32_t w, h, pad_w, pad_h;
		enc_plane_geometry(t, c, &w, &h, &pad_w, &pad_h);
		if (!q.src)
			return set_err(MIJ_E_ARG, "planes[%d].src is NULL", c);
		if (q.x_pitch <= 0 || q.x_pitch > lim || q.row_pitch < 0 || q.row_pitch > lim)
			return set_err(MIJ_E_ARG, "planes[%d]: pitch out of range (row %lld, x %lld)", c, (long long)q.row_pitch, (long long)q.x_pitch);
		if (cv && (!std::isfinite(cv->scale[c]) || !std::isfinite(cv->bias[c])))
			return set_err(MIJ_E_ARG, "scale / bias of component %d is not finite", c);
		if (!device)
			continue;
		const int64_t line = (int64_t)(w - 1) * q.x_pitch + 1;
		if (h > 1 && q.row_pitch < line)
			return set_err(MIJ_E_ARG, "planes[%d]: a row pitch of %lld lets its %lld-byte rows overlap", c, (long long)q.row_pitch, (long long)line);
		char what[16];
		snprintf(what, sizeof(what), "planes[%d]", c);
		const int rc = device_extent(e->ctx->device, q.src, (uint64_t)((int64_t)(h - 1) * q.row_pitch + line), what);
		if (rc != MIJ_OK)
			return rc;
	}
	const int flip = p->flip_vertically ? 1 : 0;
	const int slot = enc_add_common(e, t, nullptr, flip, -1, device ? ENC_DEVICE : ENC_HOST, true, true);
	if (slot < 0)
		return slot;
	EncSlot &s = e->slots[(size_t)slot];
	if (device) {
		memcpy(s.pl, p->planes, sizeof(s.pl));
		if (cv) {
			s.cv = *cv;
			s.pl_convert = true;
		}
	} else {
		enc_stage_planes(e->stage.h + s.stage_off, t, p->planes, cv, flip);
	}
	return slot;
}
extern "C" int mij_enc_add_planes(mij_encoder *e, const mij_in_planes *p, int quality) { return enc_add_planes(e, p, quality, false); }
extern "C" int mij_enc_add_device_planes(mij_encoder *e, const mij_in_planes *p, int quality) { return enc_add_planes(e, p, quality, true); }

/* A slot has a header of its own unless it is a plain clone of a plain root, which shares the root's: k_emit_build writes an optimised
 * slot's DHT segment into its header. */
static bool enc_own_header(const mij_encoder *e, const EncSlot &s)
{
	return s.clone_of < 0 || s.optimize || e->slots[(size_t)s.clone_of].optimize || s.restart != e->slots[(size_t)s.clone_of].restart || s.progressive ||
			 e->slots[(size_t)s.clone_of].progressive || s.arith != e->slots[(size_t)s.clone_of].arith;
}

/* A progressive slot's geometry as its scans see it (include/mij_host.h, PROGRESSIVE STREAMS):
 * the units (a DC scan) or blocks (an AC scan: the component's own grid, without MCU padding) scan `sc` visits, and the grid's columns */
static size_t enc_prog_scan_blocks(const mjw_tplan &t, const ProgScanDef &sc, uint32_t *bw)
{
	const bool own_grid = sc.comp == 0 && t.ncomp == 3; /* luma of a colour picture; chroma and grey have the MCU grid */
	const size_t w = own_grid ? ((size_t)t.plan.width + 7) / 8 : (size_t)t.plan.mcu_x, h = own_grid ? ((size_t)t.plan.height + 7) / 8 : (size_t)t.plan.mcu_y;
	*bw = (uint32_t)w;
	return sc.ss == 0 ? mjw_plan_du_count(&t.plan) : w * h;
}
static size_t enc_prog_tile_count(const EncSlot &s, size_t *flag_bytes)
{
	const mjw_tplan &t = s.tp;
	const int grey = t.ncomp == 1, nscan = grey ? MJW_PROGRESSIVE_SCANS_GREY : MJW_PROGRESSIVE_SCANS_COLOUR;
	size_t tiles = 0, fb = 0;
	for (int k = 0; k < nscan; ++k) {
		uint32_t bw;
		const size_t nb = enc_prog_scan_blocks(t, k_prog_script_host[grey][k], &bw);
		tiles += (nb + MIJ_EMIT_TILE - 1) / MIJ_EMIT_TILE;
		fb += k_prog_script_host[grey][k].ss ? nb : 0;
	}
	if (flag_bytes)
		*flag_bytes = fb;
	return tiles;
}

/* The tiles of a slot's nu units: MIJ_EMIT_TILE units each, cut at every end of a restart interval of ri MCUs (dpm units each) so that no tile
 * straddles one.  f(first unit, EmitTile.pad) per tile, in order; returns their number. */
template <typename F>
static size_t enc_slot_tiles(size_t nu, uint32_t dpm, uint32_t ri, F f)
{
	const size_t iu = ri ? (size_t)ri * dpm : nu;
	size_t count = 0;
	uint32_t k = 0;
	for (size_t start = 0; start < nu; start += iu, ++k) {
		const size_t stop = std::min(nu, start + iu);
		for (size_t u = start; u < stop; u += MIJ_EMIT_TILE, ++count) {
			const size_t n = std::min((size_t)MIJ_EMIT_TILE, stop - u);
			f((uint32_t)u, emit_tile_pad((uint32_t)n, u == start, u + n == stop, ri && u + n == stop && stop < nu, k));
		}
	}
	return count;
}
static size_t enc_slot_tile_count(const EncSlot &s)
{
	if (s.progressive)
		return enc_prog_tile_count(s, nullptr);
	const size_t nu = mjw_plan_du_count(&s.tp.plan), iu = s.restart ? (size_t)s.restart * (size_t)s.tp.plan.du_per_mcu : nu;
	if (!s.restart || iu >= nu)
		return (nu + MIJ_EMIT_TILE - 1) / MIJ_EMIT_TILE;
	return nu / iu * ((iu + MIJ_EMIT_TILE - 1) / MIJ_EMIT_TILE) + (nu % iu + MIJ_EMIT_TILE - 1) / MIJ_EMIT_TILE;
}

/* Emission lists at upload: one EmitSlot per slot, its tiles of MIJ_EMIT_TILE units, its headers (enc_own_header).  Optimised slots also get their tiles in a list of their
 * own, a table entry and counts. */
static int enc_emit_lists(mij_encoder *e)
{
	const size_t n = e->slots.size();
	size_t nt = 0, nh = 0, no = 0, not_ = 0, np = 0, npt = 0, nfl = 0;
	for (const EncSlot &s : e->slots) {
		const size_t tiles = enc_slot_tile_count(s);
		nt += tiles;
		nh += enc_own_header(e, s);
		if (s.progressive) { /* progressive implies its own per-scan tables: the slot is not in the optimised list */
			size_t fb = 0;
			(void)enc_prog_tile_count(s, &fb);
			++np;
			npt += tiles;
			nfl += fb;
			continue;
		}
		no += s.optimize;
		not_ += s.optimize ? tiles : 0;
	}
	const size_t ntab = no + 1 + np * MIJ_PROG_SCANS, nq = np * MIJ_PROG_SCANS;
	if (nt > UINT32_MAX)
		return set_err(MIJ_E_ARG, "too many data units to emit in one launch");
	EncEmit &m = e->em;
	Grow grow(e->stream); /* the buffers may still be in use by an earlier launch */
	grow(m.eslot, n);
	if (no) {
		grow(m.otile, not_);
		grow(m.optslot, no);
		grow(m.freq, no * 1024);
		grow(m.optok, no);
	}
	if (grow(m.tabs, ntab)) /* entry 0 again */
		HIP_TRY(hipMemcpy(m.tabs.d, &m.h_tabs0, sizeof(EmitTables), hipMemcpyHostToDevice));
	if (np) {
		grow(m.pslot, np);
		grow(m.ptile, npt);
		grow(m.pfl, nfl + 1);
		grow(m.phdr, nq * MIJ_PROG_HDR);
		grow(m.tsum, nt);
		grow(m.tafter, nt);
		grow(m.pfreq, nq * 1024);
		grow(m.phlen, nq);
		grow(m.pflag, n);
		grow(m.ctail, nt);
	}
	grow(m.etile, nt);
	grow(m.hdr, nh * MIJ_EMIT_HDR);
	grow(m.res, n + 1);
	grow(m.tbits, nt);
	grow(m.tff, nt);
	grow(m.tfrag, nt);
	grow(m.tboff, nt);
	grow(m.tout, nt);
	grow(m.sent, n);
	if (grow.rc != MIJ_OK)
		return grow.rc;
	std::vector<uint32_t> hdr_of(n), hlen_of(n, (uint32_t)MJW_HEADER_BYTES);
	uint32_t t = 0, h = 0, k = 0, ot = 0, pk = 0, pt = 0;
	uint64_t fl_off = 0;
	e->opt_of.assign(n, -1);
	for (size_t i = 0; i < n; ++i) {
		const EncSlot &s = e->slots[i];
		if (enc_own_header(e, s)) {
			uint8_t *hdr = m.hdr.h + (size_t)h * MIJ_EMIT_HDR;
			const bool lj = s.arith == MIJ_ARITH_LIBJPEG; /* libjpeg's framing: a DQT and a DHT segment per table */
			if (s.progressive) /* SOI .. SOF2; k_prog_build appends the first scan's tables and SOS */
				hlen_of[i] = (uint32_t)(lj ? mjw_lj_tframe_progressive(&s.tp, hdr) : mjw_tframe_progressive(&s.tp, hdr));
			else /* shorter for a grey slot; for the writer's own 4:2:0 and 4:4:4 what mjw_header_restart writes */
				hlen_of[i] = (uint32_t)(lj ? mjw_lj_theader_restart(&s.tp, s.restart, hdr) : mjw_theader_restart(&s.tp, s.restart, hdr));
			hdr_of[i] = h++;
		} else {
			hdr_of[i] = hdr_of[(size_t)s.clone_of];
			hlen_of[i] = hlen_of[(size_t)s.clone_of];
		}
		EmitSlot &es = m.eslot.h[i];
		es.du_off = s.dev.du_off;
		es.n_du = (uint32_t)mjw_plan_du_count(&s.tp.plan);
		es.dpm = (uint32_t)s.tp.plan.du_per_mcu;
		es.first_tile = t;
		es.n_tiles = (uint32_t)enc_slot_tile_count(s);
		es.hdr = hdr_of[i];
		es.ri = (uint32_t)s.restart;
		es.prog = 0;
		es.lj = s.arith == MIJ_ARITH_LIBJPEG;
		es.pad = 0;
		es.tab = 0;
		es.ny = s.tp.ncomp == 1 ? 1u : (uint32_t)(s.tp.lh * s.tp.lv);
		es.hlen = hlen_of[i];
		if (s.progressive) { /* its tiles name (scan, first block, count); a scan is a segment as a restart interval is */
			const mjw_tplan &tp = s.tp;
			ProgSlot &ps = m.pslot.h[pk];
			memset(&ps, 0, sizeof(ps));
			ps.slot = (uint32_t)i;
			ps.grey = tp.ncomp == 1;
			ps.nscan = ps.grey ? MJW_PROGRESSIVE_SCANS_GREY : MJW_PROGRESSIVE_SCANS_COLOUR;
			ps.lh = ps.grey ? 1u : (uint32_t)tp.lh;
			ps.lv = ps.grey ? 1u : (uint32_t)tp.lv;
			ps.mcu_x = (uint32_t)tp.plan.mcu_x;
			ps.frame_len = hlen_of[i];
			ps.tab0 = (uint32_t)(no + 1 + (size_t)pk * MIJ_PROG_SCANS);
			es.prog = ++pk;
			for (uint32_t sc = 0; sc < ps.nscan; ++sc) {
				const ProgScanDef &def = k_prog_script_host[ps.grey][sc];
				const size_t nb = enc_prog_scan_blocks(tp, def, &ps.bw[sc]);
				ps.tile0[sc] = t;
				ps.flag_off[sc] = fl_off;
				fl_off += def.ss ? nb : 0;
				for (size_t b = 0; b < nb; b += MIJ_EMIT_TILE) {
					const size_t cnt = std::min((size_t)MIJ_EMIT_TILE, nb - b);
					const bool last = b + cnt == nb;
					const EmitTile tl = {(uint32_t)i, (uint32_t)b, 0u, emit_tile_pad((uint32_t)cnt, b == 0, last, last && sc + 1 < ps.nscan, 0u) | sc << 16};
					m.ptile.h[pt++] = t;
					m.etile.h[t++] = tl;
				}
			}
			for (uint32_t sc = ps.nscan; sc <= MIJ_PROG_SCANS; ++sc)
				ps.tile0[sc] = t;
			continue;
		}
		if (s.optimize) {
			e->opt_of[i] = (int)k;
			m.optslot.h[k] = (uint32_t)i;
			es.tab = ++k;
		}
		enc_slot_tiles(es.n_du, es.dpm, es.ri, [&](uint32_t u, uint32_t pad) {
			const EmitTile tl = {(uint32_t)i, u, 0u, pad};
			m.etile.h[t++] = tl;
			if (s.optimize)
				m.otile.h[ot++] = tl;
		});
	}
	m.n_etile = nt;
	m.n_opt = no;
	m.n_otile = not_;
	m.n_prog = np;
	m.n_ptile = npt;
	if (np) {
		HIP_TRY(hipMemcpyAsync(m.pslot.d, m.pslot.h, sizeof(ProgSlot) * np, hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(m.ptile.d, m.ptile.h, sizeof(uint32_t) * npt, hipMemcpyHostToDevice, e->stream));
	}
	if (no) {
		HIP_TRY(hipMemcpyAsync(m.otile.d, m.otile.h, sizeof(EmitTile) * not_, hipMemcpyHostToDevice, e->stream));
		HIP_TRY(hipMemcpyAsync(m.optslot.d, m.optslot.h, sizeof(uint32_t) * no, hipMemcpyHostToDevice, e->stream));
	}
	HIP_TRY(hipMemcpyAsync(m.eslot.d, m.eslot.h, sizeof(EmitSlot) * n, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(m.etile.d, m.etile.h, sizeof(EmitTile) * nt, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(m.hdr.d, m.hdr.h, (size_t)nh * MIJ_EMIT_HDR, hipMemcpyHostToDevice, e->stream));
	return MIJ_OK;
}

/* The six emission launches behind the transform (mij_emit_kernels.h); with optimised slots, their counts and tables first. */
static int enc_emit_launch(mij_encoder *e)
{
	const EncEmit &m = e->em;
	const uint32_t n = (uint32_t)e->slots.size();
	const dim3 tiles((unsigned)m.n_etile), per_slot((n + 3) / 4), block(256);
	const uint8_t *du = e->du.d;
	if (m.n_opt) {
		HIP_TRY(hipMemsetAsync(m.freq.d, 0, sizeof(uint32_t) * 1024 * m.n_opt, e->stream));
		hipLaunchKernelGGL(k_emit_hist, dim3((unsigned)m.n_otile), block, 0, e->stream, m.eslot.d, m.otile.d, du, m.freq.d);
		hipLaunchKernelGGL(k_emit_build, dim3((unsigned)m.n_opt), block, 0, e->stream, m.eslot.d, m.etile.d, m.optslot.d, m.freq.d, m.tabs.d, m.hdr.d,
								 m.optok.d);
	}
	ProgArgs pa = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	if (m.n_prog) { /* block flags, run lengths, per-scan counts, per-scan tables and headers: four launches whatever the slots and scans */
		const size_t nq = m.n_prog * MIJ_PROG_SCANS;
		HIP_TRY(hipMemsetAsync(m.pfreq.d, 0, sizeof(uint32_t) * 1024 * nq, e->stream));
		HIP_TRY(hipMemsetAsync(m.phlen.d, 0, sizeof(uint32_t) * nq, e->stream));
		HIP_TRY(hipMemsetAsync(m.pflag.d, 0, sizeof(uint32_t) * n, e->stream));
		hipLaunchKernelGGL(k_prog_flags, dim3((unsigned)m.n_ptile), block, 0, e->stream, m.eslot.d, m.etile.d, m.ptile.d, m.pslot.d, du, m.pfl.d, m.tsum.d);
		hipLaunchKernelGGL(k_prog_runs, dim3((unsigned)((m.n_prog + 3) / 4)), block, 0, e->stream, m.eslot.d, m.etile.d, m.pslot.d, (uint32_t)m.n_prog,
								 m.tsum.d, m.tafter.d);
		hipLaunchKernelGGL(k_prog_hist, dim3((unsigned)m.n_ptile), block, 0, e->stream, m.eslot.d, m.etile.d, m.ptile.d, m.pslot.d, du, m.pfl.d, m.tafter.d,
								 m.pfreq.d, m.pflag.d);
		hipLaunchKernelGGL(k_prog_build, dim3((unsigned)nq), block, 0, e->stream, m.eslot.d, m.etile.d, m.pslot.d, m.pfreq.d, m.tabs.d, m.hdr.d, m.phdr.d,
								 m.phlen.d, m.pflag.d);
		pa.slots = m.pslot.d;
		pa.fl = m.pfl.d;
		pa.after = m.tafter.d;
		pa.hdr = m.phdr.d;
		pa.hlen = m.phlen.d;
		pa.ctail = m.ctail.d;
	}
	hipLaunchKernelGGL(k_emit_len, tiles, block, 0, e->stream, m.eslot.d, m.etile.d, m.tabs.d, du, m.tbits.d, pa);
	hipLaunchKernelGGL(k_emit_scan, per_slot, block, 0, e->stream, m.eslot.d, m.etile.d, n, m.tbits.d, m.tboff.d);
	hipLaunchKernelGGL(k_emit_count, tiles, block, 0, e->stream, m.eslot.d, m.etile.d, m.tabs.d, du, m.tbits.d, m.tboff.d, m.tff.d, m.tfrag.d,
							 e->has_coef ? e->sflag_dev.d : nullptr, m.n_prog ? m.pflag.d : nullptr, pa);
	hipLaunchKernelGGL(k_emit_stuff, per_slot, block, 0, e->stream, m.eslot.d, m.etile.d, n, m.tbits.d, m.tboff.d, m.tff.d, m.tfrag.d, m.tout.d, m.sent.d,
							 pa);
	hipLaunchKernelGGL(k_emit_place, dim3(1), dim3(1024), 0, e->stream, m.eslot.d, n, m.sent.d, (uint64_t)m.arena.cap, m.res.d);
	hipLaunchKernelGGL(k_emit_write, tiles, block, 0, e->stream, m.eslot.d, m.etile.d, m.tabs.d, du, m.hdr.d, m.tbits.d, m.tboff.d, m.tfrag.d,
							 m.tout.d, m.res.d, m.arena.d, pa);
	HIP_TRY(hipGetLastError());
	e->emit_queued = true;
	return MIJ_OK;
}

extern "C" int mij_enc_stream_reserve(mij_encoder *e, size_t bytes)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	HIP_TRY(hipSetDevice(e->ctx->device));
	HIP_TRY(hipStreamSynchronize(e->stream));
	enc_free_emit(e);
	e->uploaded = e->launched = false; /* the emission lists are built at upload */
	if (!bytes)
		return MIJ_OK;
	uint16_t code[4][256];
	uint8_t len[4][256];
	mjw_huff_tables(code, len);
	EmitTables &tabs = e->em.h_tabs0;
	memcpy(tabs.code, code, sizeof(code));
	memcpy(tabs.len, len, sizeof(len));
	hipError_t r = e->em.arena.alloc(bytes);
	if (r == hipSuccess)
		r = e->em.tabs.alloc(1);
	if (r == hipSuccess)
		r = hipMemcpy(e->em.tabs.d, &tabs, sizeof(tabs), hipMemcpyHostToDevice);
	if (r != hipSuccess) {
		enc_free_emit(e);
		return set_err(r == hipErrorOutOfMemory ? MIJ_E_NOMEM : MIJ_E_HIP, "mij_enc_stream_reserve(%zu): %s", bytes, hipGetErrorString(r));
	}
	return MIJ_OK;
}

extern "C" int mij_enc_fetch_streams(mij_encoder *e)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	if (!e->em.arena.d)
		return set_err(MIJ_E_STATE, "mij_enc_fetch_streams without an emission arena (mij_enc_stream_reserve)");
	if (!e->launched || !e->emit_queued)
		return set_err(MIJ_E_STATE, "mij_enc_fetch_streams before mij_enc_launch");
	HIP_TRY(hipSetDevice(e->ctx->device));
	const size_t n = e->slots.size();
	HIP_TRY(hipMemcpyAsync(e->em.res.h, e->em.res.d, sizeof(EmitResult) * (n + 1), hipMemcpyDeviceToHost, e->stream));
	HIP_TRY(hipStreamSynchronize(e->stream));
	const size_t used = (size_t)e->em.res.h[n].off;
	if (used > e->em.arena.cap)
		return set_err(MIJ_E_HIP, "emission reported %zu bytes for a %zu-byte arena", used, e->em.arena.cap);
	if (used) {
		HIP_TRY(hipMemcpyAsync(e->em.arena.h, e->em.arena.d, used, hipMemcpyDeviceToHost, e->stream));
		HIP_TRY(hipStreamSynchronize(e->stream));
	}
	e->sflag.assign(n, 0u);
	if (e->has_coef)
		HIP_TRY(hipMemcpy(e->sflag.data(), e->sflag_dev.d, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
	e->pflag.assign(n, 0u);
	if (e->em.n_prog)
		HIP_TRY(hipMemcpy(e->pflag.data(), e->em.pflag.d, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
	e->opt_ok.assign(e->em.n_opt, 0u);
	if (e->em.n_opt)
		HIP_TRY(hipMemcpy(e->opt_ok.data(), e->em.optok.d, sizeof(uint32_t) * e->em.n_opt, hipMemcpyDeviceToHost));
	e->streams_fetched = true;
	return (int)e->em.res.h[n].len;
}

extern "C" const unsigned char *mij_enc_stream(const mij_encoder *e, int slot, size_t *len)
{
	if (len)
		*len = 0;
	if (!enc_slot(e, slot))
		return nullptr;
	if (!e->streams_fetched) {
		set_err(MIJ_E_STATE, "mij_enc_stream before mij_enc_fetch_streams");
		return nullptr;
	}
	const EmitResult &r = e->em.res.h[slot];
	if (len)
		*len = (size_t)r.len;
	if (r.off == ~0ull) {
		set_err(MIJ_E_NOMEM, "slot %d did not fit in the emission arena (needs %llu bytes)", slot, (unsigned long long)r.len);
		return nullptr;
	}
	return e->em.arena.h + r.off;
}

/* mij_enc_add_device (cv NULL: uint8 elements) and mij_enc_add_device_float: the checks they share, extents in bytes of the element */
static int enc_add_device(mij_encoder *e, const mij_in_tensor *t, const mij_in_convert *cv, int quality, int flip_vertically, const mij_enc_opts *opts)
{
	if (!e || !t)
		return set_err(MIJ_E_ARG, "bad argument");
	const uint64_t es = !cv ? 1u : cv->dtype == MIJ_DT_F32 ? 4u : 2u;
	if (t->layout != MIJ_LAYOUT_HWC && t->layout != MIJ_LAYOUT_CHW)
		return set_err(MIJ_E_ARG, "mij_enc_add_device: layout %d unknown", t->layout);
	mjw_tplan plan;
	if (!enc_opts_plan(&plan, t->width, t->height, t->comp, quality, opts))
		return set_err(MIJ_E_ARG, "bad image arguments (%dx%dx%d)%s", t->width, t->height, t->comp, enc_opts_given(opts) ? ", sampling or tables" : "");
	const bool chw = t->layout == MIJ_LAYOUT_CHW;
	const int64_t w = t->width, h = t->height, C = t->comp, rp = t->row_pitch, pp = chw ? t->plane_pitch : 0;
	const int64_t lim = (int64_t)1 << 40;
	if (rp < 0 || rp > lim || pp < 0 || pp > lim)
		return set_err(MIJ_E_ARG, "pitch out of range (row %lld, plane %lld)", (long long)rp, (long long)pp);
	const int64_t line = chw ? w : w * C;
	if ((h > 1 && rp < line) || (chw && C > 1 && pp < (h - 1) * rp + w))
		return set_err(MIJ_E_ARG, "pitches let rows or planes overlap (row %lld, plane %lld; %lldx%lldx%lld %s)", (long long)rp, (long long)pp, (long long)w,
							(long long)h, (long long)C, chw ? "CHW" : "HWC");
	if (!t->src)
		return set_err(MIJ_E_ARG, "src is NULL");
	if ((uintptr_t)t->src % es)
		return set_err(MIJ_E_ARG, "src %p is not aligned to its %llu-byte elements", t->src, (unsigned long long)es);
	const uint64_t last = (uint64_t)((h - 1) * rp + (chw ? (C - 1) * pp + w - 1 : w * C - 1));
	const int rc = device_extent(e->ctx->device, t->src, (last + 1) * es, "src");
	if (rc != MIJ_OK)
		return rc;
	const int slot = enc_add_common(e, plan, nullptr, flip_vertically ? 1 : 0, -1, ENC_DEVICE, enc_opts_given(opts));
	if (slot >= 0) {
		e->slots[(size_t)slot].in = *t;
		if (cv)
			e->slots[(size_t)slot].cv = *cv;
	}
	return slot;
}

extern "C" int mij_enc_add_device_ex(mij_encoder *e, const mij_in_tensor *t, int quality, int flip_vertically, const mij_enc_opts *opts)
{
	return enc_add_device(e, t, nullptr, quality, flip_vertically, opts);
}
extern "C" int mij_enc_add_device(mij_encoder *e, const mij_in_tensor *t, int quality, int flip_vertically)
{
	return enc_add_device(e, t, nullptr, quality, flip_vertically, nullptr);
}

extern "C" int mij_enc_add_device_float(mij_encoder *e, const mij_in_tensor *t, const mij_in_convert *cv, int quality, int flip_vertically)
{
	return mij_enc_add_device_float_ex(e, t, cv, quality, flip_vertically, nullptr);
}
extern "C" int mij_enc_add_device_float_ex(mij_encoder *e, const mij_in_tensor *t, const mij_in_convert *cv, int quality, int flip_vertically,
                                           const mij_enc_opts *opts)
{
	if (!e || !t || !cv)
		return set_err(MIJ_E_ARG, "bad argument");
	if (cv->dtype != MIJ_DT_F16 && cv->dtype != MIJ_DT_BF16 && cv->dtype != MIJ_DT_F32)
		return set_err(MIJ_E_ARG, "mij_enc_add_device_float: dtype %d is not a float type%s", cv->dtype,
							cv->dtype == MIJ_DT_U8 ? " (uint8 pictures go through mij_enc_add_device)" : "");
	for (int c = 0; c < t->comp && c < 4; ++c)
		if (!std::isfinite(cv->scale[c]) || !std::isfinite(cv->bias[c]))
			return set_err(MIJ_E_ARG, "mij_enc_add_device_float: scale / bias of channel %d is not finite", c);
	return enc_add_device(e, t, cv, quality, flip_vertically, opts);
}

extern "C" int mij_enc_add_units(mij_encoder *e, int width, int height, int comp, int quality, const int16_t *du)
{
	if (!e || !du)
		return set_err(MIJ_E_ARG, "bad argument");
	mjw_tplan t;
	if (!enc_opts_plan(&t, width, height, comp, quality, nullptr))
		return set_err(MIJ_E_ARG, "bad image arguments (%dx%dx%d)", width, height, comp);
	const size_t nu = mjw_plan_du_count(&t.plan);
	const int dpm = t.plan.du_per_mcu;
	int pred[3] = {0, 0, 0};
	for (size_t u = 0; u < nu; ++u) {
		const int p = (int)(u % (size_t)dpm), c = dpm == 6 ? (p < 4 ? 0 : p - 3) : p;
		const int16_t *d = du + u * 64;
		const int diff = d[0] - pred[c];
		pred[c] = d[0];
		if (diff < -2047 || diff > 2047)
			return set_err(MIJ_E_ARG, "unit %zu: DC difference %d outside -2047..2047", u, diff);
		for (int k = 1; k < 64; ++k)
			if (d[k] < -1023 || d[k] > 1023)
				return set_err(MIJ_E_ARG, "unit %zu: AC value %d outside -1023..1023", u, d[k]);
	}
	std::vector<int16_t> units;
	try {
		units.assign(du, du + nu * 64);
	} catch (const std::bad_alloc &) {
		return set_err(MIJ_E_NOMEM, "out of host memory");
	}
	const int slot = enc_add_common(e, t, nullptr, 0, -1, ENC_UNITS);
	if (slot >= 0)
		e->slots[(size_t)slot].units.swap(units);
	return slot;
}

/* ---- coefficient slots (lossless transcode): a decode batch's planes become the slot's data units on the device */

extern "C" int mij_enc_add_coef_window(mij_encoder *e, mij_batch *b, int slot, int orientation, int trim, const int *crop, int grey,
                                       const unsigned char *luma, const unsigned char *chroma, int coarsen_only, int *rect_out)
{
	if (!e || !b)
		return set_err(MIJ_E_ARG, "bad argument");
	if (b->ctx != e->ctx)
		return set_err(MIJ_E_ARG, "mij_enc_add_coef: the batch belongs to another context");
	if (slot < 0 || slot >= (int)b->slots.size())
		return set_err(MIJ_E_ARG, "mij_enc_add_coef: bad batch slot %d", slot);
	const Slot &bs = b->slots[(size_t)slot];
	if (bs.desc.flags & MIJ_FLAG_SKIP)
		return set_err(MIJ_E_ARG, "mij_enc_add_coef: batch slot %d was rejected by the entropy stage", slot);
	if (!b->uploaded)
		return set_err(MIJ_E_ARG, "mij_enc_add_coef: the planes of batch slot %d are not in device memory yet (mij_batch_upload first)", slot);
	if (!luma != !chroma)
		return set_err(MIJ_E_ARG, "mij_enc_add_coef_requant: one table without the other");
	/* the source's plan (the planes' geometry), the grey one, the oriented one, the cropped one, and the destination's (the stream's) */
	mjw_tplan sp, gp, op, cp, tp;
	const char *why = nullptr;
	if (!mjw_tplan_from_desc(&sp, &bs.desc, &why))
		return set_err(MIJ_E_ARG, "not transcodable: %s", why ? why : "refused");
	const bool greyed = grey && sp.ncomp == 3;
	gp = sp;
	if (greyed && !mjw_tplan_grey(&gp, &sp))
		return set_err(MIJ_E_ARG, "not transcodable: bad source plan");
	if (!mjw_tplan_oriented(&op, &gp, orientation, trim, &why))
		return set_err(MIJ_E_ARG, "not transformable: %s", why ? why : "refused");
	cp = op;
	int rect[4] = {0, 0, op.plan.width, op.plan.height};
	if (crop && !mjw_tplan_cropped(&cp, &op, crop[0], crop[1], crop[2], crop[3], rect, &why))
		return set_err(MIJ_E_ARG, "not croppable: %s", why ? why : "refused");
	const bool cropped = rect[0] || rect[1] || rect[2] != op.plan.width || rect[3] != op.plan.height;
	tp = cp;
	int rq = 1; /* mjw_tplan_requant's answer: 2 where a table entry changes */
	if (luma && !(rq = mjw_tplan_requant(&tp, &cp, luma, chroma, coarsen_only, &why)))
		return set_err(MIJ_E_ARG, "not requantisable: %s", why ? why : "refused");
	const size_t nu = mjw_tplan_du_count(&tp);
	if (mjw_tplan_du_count(&sp) > UINT32_MAX / 64)
		return set_err(MIJ_E_ARG, "not transcodable: too many data units");
	const int es = enc_add_common(e, tp, nullptr, 0, -1, ENC_COEF);
	if (es < 0)
		return es;
	EncSlot &s = e->slots[(size_t)es];
	s.src = b;
	s.coef_fmt = bs.coef_bytes_fmt ? 1 : 0;
	memcpy(s.rect, rect, sizeof(rect));
	s.greyed = greyed;
	for (int c = 0; c < tp.ncomp; ++c) {
		s.coef.coef_off[c] = bs.dev.comp[c].coef_off;
		s.coef.dc_off[c] = bs.dev.comp[c].dc_off;
		s.coef.hi_off[c] = bs.dev.comp[c].hi_off;
	}
	const bool tr = orient_tr[orientation];
	s.coef.du_off = s.dev.du_off;
	s.coef.mcu_x = (uint32_t)sp.plan.mcu_x;
	s.coef.mcu_y = (uint32_t)sp.plan.mcu_y;
	s.coef.lh = (uint32_t)sp.lh;
	s.coef.lv = (uint32_t)sp.lv;
	s.coef.ncomp = (uint32_t)tp.ncomp;
	s.coef.dpm = (uint32_t)tp.plan.du_per_mcu;
	s.coef.n_du = (uint32_t)nu;
	s.coef.slot = (uint32_t)es;
	s.coef.d_mcu_x = (uint32_t)tp.plan.mcu_x;
	s.coef.d_mcu_y = (uint32_t)tp.plan.mcu_y;
	s.coef.d_lh = (uint32_t)tp.lh;
	s.coef.d_lv = (uint32_t)tp.lv;
	s.coef.ext_x = (uint32_t)(tr ? tp.plan.mcu_y : tp.plan.mcu_x);
	s.coef.ext_y = (uint32_t)(tr ? tp.plan.mcu_x : tp.plan.mcu_y);
	s.coef.orient = (orient_mx[orientation] ? MIJ_CONV_NX : 0u) | (orient_my[orientation] ? MIJ_CONV_NY : 0u) | (tr ? MIJ_CONV_TR : 0u);
	s.coef.rq = rq == 2 ? 1u : 0u; /* enc_coef_convert numbers the tables */
	memcpy(s.rq_from[0], cp.plan.ytab, 64);
	memcpy(s.rq_from[1], cp.plan.ctab, 64);
	s.coef.win = greyed || cropped ? 1u : 0u;
	if (s.coef.win) {
		/* the kept rectangle in MCUs of the oriented frame, taken back through the transpose and the mirrors into the (grey) source's
		 * stored frame, whose MCUs the trim kept are ext_x x ext_y; then in blocks of each component's plane */
		const uint32_t ex = (uint32_t)(tr ? op.plan.mcu_y : op.plan.mcu_x), ey = (uint32_t)(tr ? op.plan.mcu_x : op.plan.mcu_y);
		const uint32_t cx = (uint32_t)(rect[0] / (8 * op.lh)), cy = (uint32_t)(rect[1] / (8 * op.lv)), cw = (uint32_t)cp.plan.mcu_x, ch = (uint32_t)cp.plan.mcu_y;
		uint32_t gx = tr ? cy : cx, gy = tr ? cx : cy;
		const uint32_t gw = tr ? ch : cw, gh = tr ? cw : ch;
		if (orient_mx[orientation])
			gx = ex - gx - gw;
		if (orient_my[orientation])
			gy = ey - gy - gh;
		for (int k = 0; k < 2; ++k) {
			const uint32_t fh = k ? 1u : (uint32_t)gp.lh, fv = k ? 1u : (uint32_t)gp.lv;
			const bool none = k && tp.ncomp == 1; /* a grey destination keeps no chroma block */
			s.coef.w_ox[k] = gx * fh, s.coef.w_oy[k] = gy * fv;
			s.coef.w_ew[k] = none ? 0u : gw * fh, s.coef.w_eh[k] = none ? 0u : gh * fv;
		}
	}
	if (rect_out)
		memcpy(rect_out, rect, sizeof(rect));
	return es;
}

extern "C" int mij_enc_add_coef_requant(mij_encoder *e, mij_batch *b, int slot, int orientation, int trim, const unsigned char *luma,
                                        const unsigned char *chroma, int coarsen_only)
{
	return mij_enc_add_coef_window(e, b, slot, orientation, trim, nullptr, 0, luma, chroma, coarsen_only, nullptr);
}

/* the slot if it is a coefficient slot, or NULL with the error set */
static const EncSlot *enc_coef_slot(const mij_encoder *e, int slot)
{
	const EncSlot *s = enc_slot(e, slot, "bad slot, or not a coefficient slot");
	if (s && s->kind != ENC_COEF) {
		set_err(MIJ_E_ARG, "bad slot, or not a coefficient slot");
		return nullptr;
	}
	return s;
}

extern "C" int mij_enc_slot_rect(const mij_encoder *e, int slot, int rect[4])
{
	const EncSlot *s = rect ? enc_coef_slot(e, slot) : nullptr;
	if (!s)
		return set_err(MIJ_E_ARG, "bad slot, or not a coefficient slot");
	memcpy(rect, s->rect, sizeof(s->rect));
	return MIJ_OK;
}

extern "C" int mij_enc_slot_greyed(const mij_encoder *e, int slot)
{
	const EncSlot *s = enc_coef_slot(e, slot);
	return s ? (s->greyed ? 1 : 0) : MIJ_E_ARG;
}

extern "C" int mij_enc_slot_windowed(const mij_encoder *e, int slot)
{
	const EncSlot *s = enc_coef_slot(e, slot);
	return s ? (s->coef.win ? 1 : 0) : MIJ_E_ARG;
}

extern "C" int mij_enc_coef_tiles(const mij_encoder *e, uint32_t *tiles)
{
	if (!e || !tiles)
		return set_err(MIJ_E_ARG, "bad argument");
	*tiles = e->coef_tiles;
	return MIJ_OK;
}

extern "C" int mij_enc_add_coef_oriented(mij_encoder *e, mij_batch *b, int slot, int orientation, int trim)
{
	return mij_enc_add_coef_requant(e, b, slot, orientation, trim, nullptr, nullptr, 0);
}

extern "C" int mij_enc_add_coef(mij_encoder *e, mij_batch *b, int slot) { return mij_enc_add_coef_oriented(e, b, slot, 1, 0); }

extern "C" int mij_enc_tplan(const mij_encoder *e, int slot, mjw_tplan *out)
{
	const EncSlot *s = out ? enc_slot(e, slot, "bad slot, or not a coefficient slot") : nullptr;
	if (!s || (s->kind != ENC_COEF && !s->sampled)) /* every slot has a plan; the slots of mij_enc_plan keep that accessor */
		return set_err(MIJ_E_ARG, "bad slot, or not a coefficient slot");
	*out = s->tp;
	return MIJ_OK;
}

extern "C" int mij_enc_slot_requantized(const mij_encoder *e, int slot)
{
	const EncSlot *s = enc_coef_slot(e, slot);
	return s ? (s->coef.rq ? 1 : 0) : MIJ_E_ARG;
}

extern "C" int mij_enc_slot_status(const mij_encoder *e, int slot)
{
	if (!enc_slot(e, slot))
		return MIJ_E_ARG;
	if (!e->streams_fetched)
		return set_err(MIJ_E_STATE, "mij_enc_slot_status before mij_enc_fetch_streams");
	if ((size_t)slot < e->sflag.size() && e->sflag[(size_t)slot]) {
		set_err(MIJ_E_ARG, "slot %d: not codable: an AC coefficient outside -1023..1023 or a DC difference outside -2047..2047", slot);
		return MIJ_ENC_SLOT_UNCODABLE;
	}
	if ((size_t)slot < e->pflag.size() && e->pflag[(size_t)slot]) {
		set_err(MIJ_E_ARG, "slot %d: progressive with a forced EOB-run flush or a table that cannot be built: finish it on the host from its units", slot);
		return MIJ_ENC_SLOT_HOST_FLUSH;
	}
	if (e->em.res.h[slot].off == ~0ull) {
		set_err(MIJ_E_NOMEM, "slot %d did not fit in the emission arena (needs %llu bytes)", slot, (unsigned long long)e->em.res.h[slot].len);
		return MIJ_ENC_SLOT_NO_ROOM;
	}
	return MIJ_ENC_SLOT_OK;
}

extern "C" int mij_enc_coef_ms(mij_encoder *e, float *ms)
{
	if (!e || !ms)
		return set_err(MIJ_E_ARG, "bad argument");
	*ms = -1.0f;
	if (!e->conv_timed)
		return MIJ_OK;
	HIP_TRY(hipEventSynchronize(e->ev_conv1));
	HIP_TRY(hipEventElapsedTime(ms, e->ev_conv0, e->ev_conv1));
	return MIJ_OK;
}

/* k_coef_units' instances by [requantising][compact][MIJ_CONV_NX | MIJ_CONV_NY | MIJ_CONV_TR]; the windowed ones in a table of their own */
typedef void (*coef_units_fn)(const CoefSlot *, const WorkIdct *, const uint8_t *, uint8_t *, uint32_t *, const RqTable *);
#define MIJ_CONV_ROW_OF(C, R) \
	{k_coef_units<C, 0, 0, 0, R>, k_coef_units<C, 0, 1, 0, R>, k_coef_units<C, 0, 0, 1, R>, k_coef_units<C, 0, 1, 1, R>, \
	 k_coef_units<C, 1, 0, 0, R>, k_coef_units<C, 1, 1, 0, R>, k_coef_units<C, 1, 0, 1, R>, k_coef_units<C, 1, 1, 1, R>}
static const coef_units_fn k_coef_units_of[2][2][8] = {{MIJ_CONV_ROW_OF(0, 0), MIJ_CONV_ROW_OF(1, 0)}, {MIJ_CONV_ROW_OF(0, 1), MIJ_CONV_ROW_OF(1, 1)}};
#undef MIJ_CONV_ROW_OF
#define MIJ_CONV_ROW_OF(C, R) \
	{k_coef_units<C, 0, 0, 0, R, 1>, k_coef_units<C, 0, 1, 0, R, 1>, k_coef_units<C, 0, 0, 1, R, 1>, k_coef_units<C, 0, 1, 1, R, 1>, \
	 k_coef_units<C, 1, 0, 0, R, 1>, k_coef_units<C, 1, 1, 0, R, 1>, k_coef_units<C, 1, 0, 1, R, 1>, k_coef_units<C, 1, 1, 1, R, 1>}
static const coef_units_fn k_coef_units_win_of[2][2][8] = {{MIJ_CONV_ROW_OF(0, 0), MIJ_CONV_ROW_OF(1, 0)}, {MIJ_CONV_ROW_OF(0, 1), MIJ_CONV_ROW_OF(1, 1)}};
#undef MIJ_CONV_ROW_OF

/* The plane tiles of component c a slot's conversion reads: every tile of the plane for a plain slot; for a windowed one those that hold
 * a block of the kept rectangle (a tile is 64 consecutive blocks of the plane in raster order), in rising order.  Calls f(tile). */
template <typename F>
static void coef_slot_tiles(const CoefSlot &cs, uint32_t c, F f)
{
	const size_t bw = (size_t)cs.mcu_x * (c ? 1u : cs.lh), bh = (size_t)cs.mcu_y * (c ? 1u : cs.lv);
	if (!cs.win) {
		for (size_t t = 0; t < (bw * bh + 63) / 64; ++t)
			f((uint32_t)t);
		return;
	}
	const int k = c ? 1 : 0;
	size_t next = 0; /* the first tile not yet named */
	for (size_t by = cs.w_oy[k]; cs.w_ew[k] && by < (size_t)cs.w_oy[k] + cs.w_eh[k]; ++by) {
		const size_t lo = (by * bw + cs.w_ox[k]) >> 6, hi = (by * bw + cs.w_ox[k] + cs.w_ew[k] - 1) >> 6;
		for (size_t t = lo > next ? lo : next; t <= hi; ++t)
			f((uint32_t)t);
		next = hi + 1 > next ? hi + 1 : next;
	}
}

/* The conversion kernel of the coefficient slots, queued at upload in place of a copy of units: behind an event on every source
 * batch's stream, one launch per (batch, plane format, orientation's template instance, plain or requantising, whole or windowed) over a
 * list of plane tiles -- every tile of a plain slot's planes, those its kept rectangle touches for a windowed one (coef_slot_tiles).  The
 * flags are cleared whenever the emission may read them. */
static int enc_coef_convert(mij_encoder *e)
{
	const size_t n = e->slots.size();
	size_t nc = 0, nw = 0, nq = 0;
	for (const EncSlot &s : e->slots)
		if (s.kind == ENC_COEF) {
			++nc;
			nq += s.coef.rq ? 1 : 0;
			for (uint32_t c = 0; c < s.coef.ncomp; ++c) /* what is queued below: a windowed slot names only the tiles its rectangle touches */
				coef_slot_tiles(s.coef, c, [&](uint32_t) { ++nw; });
		}
	e->has_coef = nc != 0;
	e->conv_timed = false;
	e->coef_tiles = 0;
	if (!nc)
		return MIJ_OK;
	if (nw > UINT32_MAX)
		return set_err(MIJ_E_ARG, "too many plane tiles to convert in one launch");
	Grow grow(e->stream);
	grow(e->cslot, nc);
	grow(e->rqt, nq);
	grow(e->cwork, nw);
	grow(e->sflag_dev, n);
	if (grow.rc != MIJ_OK)
		return grow.rc;
	if (!e->ev_coef) {
		HIP_TRY(hipEventCreateWithFlags(&e->ev_coef, hipEventDisableTiming));
		HIP_TRY(hipEventCreate(&e->ev_conv0));
		HIP_TRY(hipEventCreate(&e->ev_conv1));
	}
	/* groups: slots of one batch, one plane format and one template instance (orientation; plain or requantising; whole or windowed) are
	 * contiguous in the lists */
	struct Group {
		mij_batch *b;
		int fmt;
		uint32_t orient;
		bool rq, win;
		size_t first, count;
	};
	std::vector<Group> groups;
	std::vector<mij_batch *> batches;
	for (const EncSlot &s : e->slots)
		if (s.kind == ENC_COEF) {
			bool seen = false;
			for (const Group &g : groups)
				seen = seen || (g.b == s.src && g.fmt == s.coef_fmt && g.orient == s.coef.orient && g.rq == (s.coef.rq != 0) && g.win == (s.coef.win != 0));
			if (!seen)
				groups.push_back(Group{s.src, s.coef_fmt, s.coef.orient, s.coef.rq != 0, s.coef.win != 0, 0, 0});
			if (std::find(batches.begin(), batches.end(), s.src) == batches.end())
				batches.push_back(s.src);
		}
	size_t k = 0, w = 0, q = 0;
	for (Group &g : groups) {
		g.first = w;
		for (const EncSlot &s : e->slots) {
			if (s.kind != ENC_COEF || s.src != g.b || s.coef_fmt != g.fmt || s.coef.orient != g.orient || g.rq != (s.coef.rq != 0) || g.win != (s.coef.win != 0))
				continue;
			e->cslot.h[k] = s.coef;
			e->cslot.h[k].ri = (uint32_t)s.restart;
			if (g.rq) {
				rq_fill(e->rqt.h[q], (s.coef.orient & MIJ_CONV_TR) != 0, s.rq_from[0], s.tp.plan.ytab, s.rq_from[1], s.tp.plan.ctab);
				e->cslot.h[k].rq = (uint32_t)++q;
			}
			for (uint32_t c = 0; c < s.coef.ncomp; ++c)
				coef_slot_tiles(s.coef, c, [&](uint32_t t) { e->cwork.h[w++] = WorkIdct{(uint32_t)k, c, t, 0u}; });
			++k;
		}
		g.count = w - g.first;
	}
	HIP_TRY(hipMemcpyAsync(e->cslot.d, e->cslot.h, sizeof(CoefSlot) * nc, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(e->cwork.d, e->cwork.h, sizeof(WorkIdct) * nw, hipMemcpyHostToDevice, e->stream));
	if (nq)
		HIP_TRY(hipMemcpyAsync(e->rqt.d, e->rqt.h, sizeof(RqTable) * nq, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemsetAsync(e->sflag_dev.d, 0, sizeof(uint32_t) * n, e->stream));
	for (mij_batch *b : batches) { /* whatever the batch's stream still does to the planes comes first */
		HIP_TRY(hipEventRecord(e->ev_coef, b->stream));
		HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_coef, 0));
	}
	HIP_TRY(hipEventRecord(e->ev_conv0, e->stream));
	for (const Group &g : groups) {
		if (!g.count)
			continue;
		const dim3 grid((unsigned)g.count), block(64);
		uint8_t *du = e->du.d;
		hipLaunchKernelGGL((g.win ? k_coef_units_win_of : k_coef_units_of)[g.rq ? 1 : 0][g.fmt ? 1 : 0][g.orient & 7u], grid, block, 0, e->stream, e->cslot.d, e->cwork.d + g.first, g.b->coef.d, du,
								 e->sflag_dev.d, static_cast<const RqTable *>(e->rqt.d));
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipEventRecord(e->ev_conv1, e->stream));
	e->coef_tiles = (uint32_t)nw;
	e->conv_timed = true;
	return MIJ_OK;
}

/* The transform group of a slot; EG_NONE for given units and for units made from coefficient planes, which have nothing to transform.  A
 * plane slot always takes its own strip kernel.  A pixel slot takes the strip kernel of its MCU shape (a sampled 4:2:0 or 4:4:4 the
 * instance a default slot takes), or under force_generic, which a sampled slot ignores, the per-unit luma kernel of its sampling: the
 * chroma one is the next group. */
static EncGroup enc_classify(const mij_encoder *e, const EncSlot &s)
{
	const mjw_tplan &t = s.tp;
	if (!enc_has_pixels(s.kind))
		return EG_NONE;
	if (s.arith == MIJ_ARITH_LIBJPEG) /* pass 2's group; a pixel slot also takes EG_LJ_PASS1 of it */
		return t.ncomp == 1 ? EG_LJGREY : t.lh == 1 ? EG_LJ444 : t.lv == 1 ? EG_LJ422 : EG_LJ420;
	if (s.planes)
		return t.ncomp == 1 ? EG_PGREY : t.lh == 2 ? (t.lv == 2 ? EG_P420 : EG_P422) : (t.lv == 2 ? EG_P440 : EG_P444);
	if (t.ncomp == 1)
		return EG_GREY;
	if (t.lh != t.lv)
		return t.lh == 2 ? EG_422 : EG_440;
	if (e->force_generic && !s.sampled)
		return t.lh == 2 ? EG_Y420 : EG_Y444;
	return t.lh == 2 ? EG_420 : EG_444;
}

extern "C" int mij_enc_upload(mij_encoder *e)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	HIP_TRY(hipSetDevice(e->ctx->device));
	const size_t n = e->slots.size();
	if (!n)
		return set_err(MIJ_E_STATE, "encoder batch is empty");
	std::vector<WorkIdct> work[EG_GROUPS];
	size_t lj_bytes = 0, n_lj = 0;
	for (const EncSlot &s : e->slots)
		n_lj += s.arith == MIJ_ARITH_LIBJPEG;
	if (n_lj) { /* one record per slot; the planes of the pixel slots among them one behind the other */
		Grow grow(e->stream);
		grow(e->lj, n);
		if (grow.rc != MIJ_OK)
			return grow.rc;
		memset(e->lj.h, 0, sizeof(LjEncSlot) * n);
	}
	for (size_t i = 0; i < n; ++i) {
		const EncSlot &s = e->slots[i];
		e->imgs.h[i] = s.dev;
		const EncGroup g = enc_classify(e, s);
		if (g == EG_NONE)
			continue;
		if (s.arith == MIJ_ARITH_LIBJPEG) {
			const mjw_tplan &t = s.tp;
			LjEncSlot &L = e->lj.h[i];
			L.from_pix = s.planes;
			L.off = lj_bytes;
			L.rw = (uint32_t)(t.plan.width + 7) / 8u;
			L.rh = (uint32_t)(t.plan.height + 7) / 8u;
			L.srows = (uint32_t)(t.plan.height + (t.ncomp == 1 ? 1 : t.lv) - 1) / (uint32_t)(t.ncomp == 1 ? 1 : t.lv);
			for (int k = 0; k < 64; ++k) { /* natural order from the tables' zigzag order */
				const int z = enc_zigzag_of[k];
				L.m[0][k] = mjw_lj_quant_magic(t.plan.ytab[z]), L.h[0][k] = 4u * t.plan.ytab[z];
				L.m[1][k] = mjw_lj_quant_magic(t.plan.ctab[z]), L.h[1][k] = 4u * t.plan.ctab[z];
			}
			const uint32_t nm = (uint32_t)(t.plan.mcu_x * t.plan.mcu_y);
			if (!s.planes) {
				lj_bytes += enc_plane_bytes(t);
				for (uint32_t cy = 0; cy < (uint32_t)t.plan.mcu_y * 8u; ++cy)
					work[EG_LJ_PASS1(g)].push_back(WorkIdct{(uint32_t)i, 0u, cy, 0u});
			}
			for (uint32_t f = 0; f < nm; f += enc_families[g].strip)
				work[g].push_back(WorkIdct{(uint32_t)i, 0u, f, 0u});
			continue;
		}
		/* a strip kernel's items count MCUs; the per-unit pair's count the luma units, and in the next group the two chroma units per MCU */
		const bool pair = g <= EG_C420;
		const uint32_t nm = (uint32_t)(s.tp.plan.mcu_x * s.tp.plan.mcu_y);
		const uint32_t count[2] = {pair ? nm * (g == EG_Y420 ? 4u : 1u) : nm, nm * 2u};
		for (uint32_t k = 0; k < (pair ? 2u : 1u); ++k)
			for (uint32_t f = 0; f < count[k]; f += enc_families[g + k].strip)
				work[g + k].push_back(WorkIdct{(uint32_t)i, k, f, 0u});
	}
	size_t total = 0;
	for (int g = 0; g < EG_GROUPS; ++g)
		total += work[g].size();
	Grow grow(e->stream);
	grow(e->work, total);
	if (lj_bytes)
		grow(e->lj_planes, lj_bytes);
	if (grow.rc != MIJ_OK)
		return grow.rc;
	if (n_lj)
		HIP_TRY(hipMemcpyAsync(e->lj.d, e->lj.h, sizeof(LjEncSlot) * n, hipMemcpyHostToDevice, e->stream));
	size_t pos = 0;
	for (int g = 0; g < EG_GROUPS; ++g) {
		e->first_work[g] = pos;
		e->n_work[g] = work[g].size();
		if (!work[g].empty())
			memcpy(e->work.h + pos, work[g].data(), work[g].size() * sizeof(WorkIdct));
		pos += work[g].size();
	}
	HIP_TRY(hipMemcpyAsync(e->imgs.d, e->imgs.h, sizeof(EncImage) * n, hipMemcpyHostToDevice, e->stream));
	HIP_TRY(hipMemcpyAsync(e->work.d, e->work.h, sizeof(WorkIdct) * total, hipMemcpyHostToDevice, e->stream));
	for (size_t i = 0; i < n; ++i) {
		const EncSlot &s = e->slots[i];
		if (s.clone_of < 0 && s.kind == ENC_HOST)
			HIP_TRY(hipMemcpyAsync(e->pix.d + s.dev.pix_off, e->stage.h + s.stage_off, s.pix_bytes, hipMemcpyHostToDevice, e->stream));
		else if (s.kind == ENC_UNITS)
			HIP_TRY(hipMemcpyAsync(e->du.d + s.dev.du_off, s.units.data(), s.units.size() * sizeof(int16_t), hipMemcpyHostToDevice, e->stream));
	}
	int rc = enc_gather(e); /* device-pixel slots, before the clones copy them */
	if (rc == MIJ_OK)
		rc = enc_gather_float(e);
	if (rc == MIJ_OK)
		rc = enc_gather_planes(e);
	if (rc == MIJ_OK)
		rc = enc_coef_convert(e);
	if (rc != MIJ_OK)
		return rc;
	for (size_t i = 0; i < n; ++i) {
		const EncSlot &s = e->slots[i];
		if (s.clone_of >= 0)
			HIP_TRY(hipMemcpyAsync(e->pix.d + s.dev.pix_off, e->pix.d + e->slots[(size_t)s.clone_of].dev.pix_off, s.pix_bytes, hipMemcpyDeviceToDevice, e->stream));
	}
	if (e->em.arena.d) {
		rc = enc_emit_lists(e);
		if (rc != MIJ_OK)
			return rc;
	}
	e->uploaded = true;
	e->launched = false;
	e->emit_queued = e->streams_fetched = false;
	return MIJ_OK;
}

extern "C" int mij_enc_launch(mij_encoder *e)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	if (!e->uploaded)
		return set_err(MIJ_E_STATE, "mij_enc_launch before mij_enc_upload");
	HIP_TRY(hipSetDevice(e->ctx->device));
	for (int g = 0; g < EG_GROUPS; ++g) {
		if (!e->n_work[g])
			continue;
		const EncFamily &f = enc_families[g];
		if (f.klj)
			hipLaunchKernelGGL(f.klj, dim3((unsigned)e->n_work[g]), dim3(f.threads), f.lds, e->stream, e->imgs.d, e->work.d + e->first_work[g], e->pix.d,
									 reinterpret_cast<int16_t *>(e->du.d), static_cast<const LjEncSlot *>(e->lj.d), e->lj_planes.d);
		else
			hipLaunchKernelGGL(f.k, dim3((unsigned)e->n_work[g]), dim3(f.threads), f.lds, e->stream, e->imgs.d, e->work.d + e->first_work[g], e->pix.d,
									 reinterpret_cast<int16_t *>(e->du.d));
		HIP_TRY(hipGetLastError());
	}
	if (e->em.arena.d) {
		const int rc = enc_emit_launch(e);
		if (rc != MIJ_OK)
			return rc;
	}
	e->launched = true;
	e->streams_fetched = false;
	return MIJ_OK;
}

extern "C" int mij_enc_force_generic(mij_encoder *e, int on)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	e->force_generic = on != 0;
	e->uploaded = e->launched = false;
	return MIJ_OK;
}

extern "C" int mij_enc_wait(mij_encoder *e)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	HIP_TRY(hipSetDevice(e->ctx->device));
	HIP_TRY(hipStreamSynchronize(e->stream));
	return MIJ_OK;
}

extern "C" int mij_enc_fetch(mij_encoder *e, int slot, int16_t *dst, size_t dst_elems)
{
	if (!e || slot < 0 || slot >= (int)e->slots.size() || !dst)
		return set_err(MIJ_E_ARG, "bad slot or destination");
	if (!e->launched)
		return set_err(MIJ_E_STATE, "mij_enc_fetch before launch");
	const EncSlot &s = e->slots[(size_t)slot];
	const size_t elems = mjw_plan_du_count(&s.tp.plan) * 64;
	if (dst_elems < elems)
		return set_err(MIJ_E_ARG, "destination too small");
	HIP_TRY(hipSetDevice(e->ctx->device));
	return d2h_bounced(e->ctx, e->stream, dst, e->du.d + s.dev.du_off, elems * 2);
}

extern "C" int mij_enc_plan(const mij_encoder *e, int slot, mjw_plan *out)
{
	if (!e || slot < 0 || slot >= (int)e->slots.size() || !out)
		return set_err(MIJ_E_ARG, "bad slot");
	*out = e->slots[(size_t)slot].tp.plan;
	return MIJ_OK;
}

extern "C" int mij_enc_timer_begin(mij_encoder *e)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	HIP_TRY(hipEventRecord(e->ev_begin, e->stream));
	return MIJ_OK;
}
extern "C" int mij_enc_timer_end(mij_encoder *e)
{
	if (!e)
		return set_err(MIJ_E_ARG, "encoder is NULL");
	HIP_TRY(hipEventRecord(e->ev_end, e->stream));
	return MIJ_OK;
}
extern "C" int mij_enc_timer_elapsed_ms(mij_encoder *e, float *ms)
{
	if (!e || !ms)
		return set_err(MIJ_E_ARG, "bad argument");
	HIP_TRY(hipEventSynchronize(e->ev_end));
	HIP_TRY(hipEventElapsedTime(ms, e->ev_begin, e->ev_end));
	return MIJ_OK;
}

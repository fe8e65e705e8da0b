/*
 * pyfocusr_hip.h — C-ABI of libpyfocusr_hip.so: the MI355X (gfx950) implementation of
 * pyfocusr's spectral-embedding hot path.
 *
 * The reference (gattia/pyfocusr) is pure Python with no FFI layer of its own; its boundary
 * for this path is the Python class API (Graph / eigsort / Focusr).  The entry points below
 * are what a ctypes binding of that path needs; each one names the reference code it
 * replaces (file:line in /root/reference/pyfocusr).  The Python mirror of the reference
 * classes that calls them lives in pyfocusr_amd/{graph,eigsort,focusr}.py; INTEGRATION.md
 * shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - plain C: pointers + sizes, no C++/torch types; all functions return 0 on success or a
 *    negative PF_E_* code (message via pf_last_error()); nothing throws.
 *  - host arrays are caller-owned, C-contiguous; the library never keeps a host pointer.
 *  - one pf_ctx per (device, HIP stream); a pf_graph belongs to the ctx that built it.  Calls
 *    on one ctx must not overlap in time; distinct ctxs are independent.
 *  - "slot" = one length-n float64 vector in the graph's device workspace.
 */
#ifndef PYFOCUSR_HIP_H
#define PYFOCUSR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PF_VERSION 1

#define PF_OK 0
#define PF_E_ARG (-1)        /* bad argument (null pointer, size, slot range, face index out of range) */
#define PF_E_HIP (-2)        /* HIP runtime error (allocation, launch, copy); see pf_last_error() */
#define PF_E_DEGENERATE (-3) /* a face repeats a vertex: the reference would store W_ii = inf; or the samples of
                                pf_fmap_zoomout_sampled do not determine the fit */
#define PF_E_STATE (-4)      /* call order violated (e.g. knn run before upload) */
#define PF_E_PERSIST_TIMEOUT (-5) /* a wait inside the resident Chebyshev kernel ran out (device shared?): the filter
                                     applications since the last synchronising call are invalid; the stream has been
                                     drained and the path switched off - repeat the solve (pf_eigs_smallest and the
                                     Python drivers do so by themselves) */
#define PF_E_INTERNAL (-6)   /* a bound that the algorithm guarantees was exceeded (pf_mesh_topology's labelling rounds) */

/* operator selector for the eigensolver kernels */
#define PF_OP_RW 0  /* L = G (D - W), G = diag(1/(deg+1e-8))   graph.py:216-226 (as stored by the reference) */
#define PF_OP_SYM 1 /* S = G^1/2 (D - W) G^1/2: same spectrum, only when W is symmetric */

typedef struct pf_ctx pf_ctx;
typedef struct pf_graph pf_graph;
typedef struct pf_mesh pf_mesh; /* points + faces resident in HBM */

typedef struct pf_graph_info {
    int64_t n;             /* vertices */
    int64_t n_faces;
    int64_t nnz_w;         /* unique directed edges = nnz(W)                       graph.py:178 */
    int64_t nnz_l;         /* nnz of scipy's L = nnz_w + #(vertices with deg>0)     graph.py:226 */
    int32_t is_symmetric;  /* W == W^T (structure; values then agree bit for bit)  */
    int32_t n_isolated;    /* vertices referenced by no face (deg == 0)            */
    int32_t n_components;  /* weakly connected components with >= 2 vertices       */
    int32_t max_degree;    /* longest row of W                                      */
    int64_t sell_entries;  /* stored off-diagonal slots incl. padding (SELL-64)     */
    int64_t n_pad;         /* workspace slot stride in elements                     */
    int64_t n_oneway;      /* entries (i,j) of W without a matching (j,i): 0 iff symmetric;
                              every boundary edge of an open mesh is one (graph.py:178)      */
    double spectral_bound; /* proven upper bound of the spectrum of L (and of S): 2 in general; for a closed triangle
                              mesh (every edge in exactly two faces) 1 + (1 + sqrt(1 - 4 P_min)) / 2 with P_min the
                              smallest 2abc / ((a+b)(a+c)(b+c)) over the faces' edge weights - the Chebyshev
                              filter damps [cut, spectral_bound] instead of [cut, 2]                  */
} pf_graph_info;

typedef struct pf_timing {
    double op_ms;        /* accumulated device time of fused SpMV/Chebyshev launches (HIP events) */
    int64_t op_launches; /* number of those launches                                              */
    double op_bytes;     /* algorithmic bytes they moved: sum of 12 nnz + 20 n + 4 per graph and step */
    double knn_ms;       /* device time of the last pf_knn_run                                    */
    double build_ms;     /* device time of the last pf_graph_build (kernels only)                 */
    /* the part of the above done by the resident kernel (pf_persist_enable): one launch = a whole recurrence */
    double persist_ms;
    int64_t persist_launches;
    int64_t persist_steps; /* recurrence steps those launches ran, summed over the graphs of a launch (graph-steps) */
    double persist_bytes;  /* algorithmic bytes, counted as for op_bytes                                   */
    double persist_lds_bytes; /* LDS bytes the resident launches moved: per graph and step 8 B per stored SELL entry
                                 (the gathered x) + 16 B per row (own x read, result written) + 8 B per outside row */
} pf_timing;

/* ---- context -------------------------------------------------------------------------- */
int pf_version(void);
/* Debugging aid, process-wide, off by default: on = 1 fills every block the library's device memory pool hands out with
 * 0xFF bytes (NaN as a floating-point number, -1 as an integer) before its first use, on the stream that asked for it;
 * on = 2 fills it with zero bytes instead (for readers of blocks that are set to all-ones on purpose); 0 is off, any
 * other value acts like 1.
 * Results do not change - nothing in the library reads pool memory it has not written - and a run that does change has
 * found a reader of uninitialised memory.  Costs one fill launch per allocation while on, nothing while off. */
int pf_pool_poison(int on);
const char* pf_last_error(void);
int pf_device_count(void);
int pf_create(int device, pf_ctx** out);
void pf_destroy(pf_ctx* ctx);
int pf_sync(pf_ctx* ctx);
void* pf_stream(pf_ctx* ctx); /* the ctx's hipStream_t, so that a peer library (RCCL through torch) can enqueue on it */
/* time operator launches with HIP events on the ctx stream: on = 1 every filter application, on = N > 1 every N-th (an
 * event record costs ~5 us of device time: two per application are 0.25 ms of a 13.5 ms pair step); the accumulated
 * figures of pf_timing_get then cover the timed applications only */
int pf_timing_enable(pf_ctx* ctx, int on);
int pf_timing_get(pf_ctx* ctx, pf_timing* out, int reset);

/* ---- Laplacian assembly --------------------------------------------------------------- */
/* Replaces Graph.get_weighted_adjacency_matrix / get_degree_matrix / get_G_matrix (no
 * features) / get_laplacian_matrix   (graph.py:148-178, 216-219, 213-214, 221-226).
 * pts: n x 3 float64; faces: F x verts_per_face int32 (VTK polygon edge order
 * (0,1),(1,2),...,(v-1,0)).  Directed "set" semantics: W[i,j] = 1/||xi-xj|| once per unique
 * directed edge.  Builds, on the device: CSR(W) with sorted columns, deg (row sums, left to
 * right in column order), the SELL-64 operator storage for L (and S when W is symmetric), and
 * connected-component labels. */
int pf_graph_build(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces,
                   int32_t verts_per_face, pf_graph** out);
/* the same in two steps: host -> HBM copy of the mesh, then assembly from resident inputs */
int pf_mesh_upload(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces,
                   int32_t verts_per_face, pf_mesh** out);
void pf_mesh_free(pf_mesh* mesh);
int pf_graph_build_device(pf_mesh* mesh, pf_graph** out);
/* The two meshes of a pair assembled side by side (mesh a on the ctx stream, mesh b on a second stream of the ctx, the
 * two builds' halves interleaved around their one synchronisation each): an assembly is ~75 small kernels that are
 * mostly launch latency, and two of them overlap almost completely.  Same results as two pf_graph_build_device calls. */
int pf_graph_build_device2(pf_mesh* mesh_a, pf_mesh* mesh_b, pf_graph** out_a, pf_graph** out_b);
/* A device graph from a general sparse matrix A in CSR (sorted, unique columns; explicit diagonal optional)
 * instead of a mesh: what `recursive_eig(matrix, ...)` (graph.py:357-389) needs when it is handed a scipy
 * matrix.  PF_OP_RW applies A itself; is_symmetric reports A == A^T numerically (PF_OP_SYM is then the same
 * operator); deg/l_diag hold the diagonal; rows without off-diagonal entries count as isolated. */
int pf_graph_from_matrix(pf_ctx* ctx, int64_t n, const int32_t* rowptr, const int32_t* colidx, const double* values,
                         pf_graph** out);
/* The cotangent Laplace-Beltrami operator of a resident triangle mesh (the reference has none: an extra).
 *   w_ij = 1/2 sum over the faces containing the undirected edge (i,j) of cot(angle opposite it), cot = (u.v)/|u x v| at
 *          the corner with edge vectors u, v; terms in ascending face index; (i,j) and (j,i) hold the same bits; negative
 *          weights (obtuse angles) are kept
 *   d_i  = sum_j w_ij left to right in column order;  m_i = 1/3 sum of the incident faces' areas (|u x v|/2 at the face's
 *          first corner) in ascending face index: the lumped barycentric mass (mass_kind 0, the only one)
 * No floating-point atomics: two builds give identical bits.  The graph's operator is the symmetric
 *   S = M^-1/2 (D - W) M^-1/2:  S_ij = -w_ij / (sqrt(m_i) sqrt(m_j)),  S_ii = d_i / m_i
 * (spectrum of the generalised problem (D - W) phi = lambda M phi, eigenvectors M^1/2 phi) stored as for
 * pf_graph_from_matrix: PF_OP_RW and PF_OP_SYM both apply S, is_symmetric = 1, pf_graph_download gives the structure with
 * w = -S_ij, deg = l_diag = S_ii; pf_graph_info.spectral_bound is the Gershgorin bound max_i sum_j |S_ij| (not <= 2).  A
 * vertex in no face (m_i = 0) has an empty row, counts in n_isolated and stays 0 in every eigenvector.
 * pf_lock_null_vectors locks sqrt(m) restricted to each component.  Rows stay in the caller's numbering (no m-space).
 * Errors: verts_per_face != 3 or a face index out of range PF_E_ARG; a face that repeats a vertex or has |u x v| == 0 (or
 * non-finite) PF_E_DEGENERATE.  Runs on the ctx stream; pf_timing.build_ms is its device time. */
int pf_graph_build_cotan(pf_mesh* mesh, int32_t mass_kind /* 0 = barycentric */, pf_graph** out);
/* hi = max_i sum_j |S_ij| (diagonal included), total_area = sum of the faces' areas (fixed order); each may be NULL */
int pf_graph_cotan_info(pf_graph* g, double* hi, double* total_area);
/* w[nnz_w] = w_ij in the CSR order of pf_graph_download, diag[n] = d_i, mass[n] = m_i; each may be NULL */
int pf_graph_cotan_download(pf_graph* g, double* w, double* diag, double* mass);
/* out = M^-1 (D - W) x for a host block x[n][ncols] (row-major, 1 <= ncols <= 8): out_i = (sum_j w_ij (x_i - x_j)) / m_i,
 * the row left to right; 0 where m_i == 0.  Applied to the points it is the mean-curvature normal (|.| = 2 H). */
int pf_cotan_apply(pf_graph* g, const double* x, int32_t ncols, double* out);
/* (the three calls above return PF_E_ARG for a graph that pf_graph_build_cotan did not build) */
void pf_graph_free(pf_graph* g);
int pf_graph_get_info(pf_graph* g, pf_graph_info* out);
/* 1 if the mesh this graph was built from listed a directed edge more than once (duplicated faces, non-manifold edges):
 * the build then moved the rows of CSR(W) together after dropping the repeats.  0 for every closed manifold mesh - the
 * sorted rows are CSR(W) as they stand and that pass returns at once - and for graphs not built from a mesh. */
int pf_graph_rows_compacted(pf_graph* g);
/* CSR(W): rowptr[n+1], colidx[nnz_w], w[nnz_w]; l_offdiag[nnz_w] = -w/(deg_i+1e-8);
 * per-vertex deg[n], l_diag[n] = deg/(deg+1e-8).  Any output may be NULL. */
int pf_graph_download(pf_graph* g, int32_t* rowptr, int32_t* colidx, double* w, double* l_offdiag,
                      double* deg, double* l_diag, int32_t* component_label);

/* ---- device workspace ------------------------------------------------------------------ */
int pf_ws_ensure(pf_graph* g, int32_t n_slots);
int pf_ws_upload(pf_graph* g, int32_t slot, const double* x);            /* x[n]            */
int pf_ws_download(pf_graph* g, int32_t first, int32_t count, double* out); /* out[count][n]  */
int pf_ws_copy(pf_graph* g, int32_t src, int32_t dst, int32_t count);
/* Krylov start vector into `slot`: a low-order polynomial of the vertex positions (rich in the low
 * eigenmodes) plus counter-based noise from `seed`; zero on isolated vertices.  Deterministic. */
int pf_start_vector(pf_graph* g, int32_t slot, uint64_t seed);
int pf_mask_isolated(pf_graph* g, int32_t slot);                          /* x[i] = 0 where deg_i == 0 */
/* unit-norm null vectors of `op`, one per component with >= 2 vertices, into slots
 * [0, n_components): 1_C for PF_OP_RW, sqrt(deg+1e-8) on C for PF_OP_SYM; sqrt(m) on C for a cotangent graph. */
int pf_lock_null_vectors(pf_graph* g, int32_t op, int32_t* n_locked);

/* ---- eigensolver kernels (replace scipy eigs/ARPACK+SuperLU at graph.py:372) ------------- */
int pf_spmv(pf_graph* g, int32_t op, int32_t src, int32_t dst);           /* dst = A src     */
/* slots [dst_first, dst_first+count) = A slots [src_first, src_first+count), one call (the Rayleigh-Ritz step's A Z) */
int pf_spmv_multi(pf_graph* g, int32_t op, int32_t src_first, int32_t dst_first, int32_t count);
/* dst = T_degree((c I - A)/e) src / rho^degree : `degree` launches of the fused SpMV + three-term
 * recurrence kernel (scaled by rho >= 1 per step so that high degrees cannot overflow; rho = 1 is the
 * plain Chebyshev polynomial).  src is preserved; dst != src. */
/* ON by default: pf_cheb / pf_cheb2 run the WHOLE recurrence in one resident kernel (one block per CU) when the
 * graph(s) fit: each block owns a window of 1024 / 2048 / 4096 consecutive rows of every graph, keeps the rows' entries
 * in registers and the window's x in LDS, and neighbouring windows hand their boundary rows over through memory, one
 * value per outside row, no flags (pf_persist.hip; graphs up to 256 windows: ~1M rows, pairs up to ~524k rows each).
 * Everything else runs one step per launch.  Results are bit-identical in all cases.  0 switches it off (also:
 * environment PF_PERSIST=0); process-wide.  Needs 4 x n_pad doubles of scratch per graph.  All blocks must be resident
 * together (grid <= CU count; an idle device): a wait that runs out (another tenant on the device) is reported as
 * PF_E_PERSIST_TIMEOUT at the next synchronising call, after the library has drained the stream and SUSPENDED the path:
 * the next 64 filter applications run one step per launch, then the resident path is tried again (every further timeout
 * doubles the suspension; pf_persist_enable(1) lifts it; pf_persist_state tells).  One ctx has resident kernels in
 * flight at a time: the path belongs to the ctx that used it last, another ctx takes it over as soon as the owner's
 * last resident launch has completed and runs one step per launch until then. */
int pf_persist_enable(int on);
/* Level 1 by default: single-graph recurrences (pf_cheb) on graphs with windows of 1024 rows (up to ~262k rows) whose
 * windows see each other symmetrically (any symmetric W) exchange boundary values every SECOND step: a window repeats
 * the odd steps of the outside rows it reads itself (k_cheb_resident2: one memory-side hand-off per two steps; 250k
 * rows: 1.41 -> 1.24 us per step).  Paired recurrences (pf_cheb2) always take one step per exchange: two steps were
 * measured slower there (2.08 against 1.85 us per step of a 250k pair).  0: one step per exchange everywhere; any level
 * above 1 means 1.  Bit-identical results at every level.  Environment: PF_PERSIST_S2=0/1; process-wide. */
int pf_persist_two_step(int level);
/* On by default: a paired recurrence (pf_cheb2) on windows of 1024 rows whose outside-row lists fit half a block runs the
 * kernel whose two halves take the graphs in opposite order (k_cheb_resident<2,1,8,true>), so that both graphs'
 * boundary rows are handed over one row's latency into a step.  0: both graphs in the same order everywhere.
 * Bit-identical results either way.  Environment: PF_PERSIST_HALVES=0/1; process-wide. */
int pf_persist_pair_halves(int on);
/* The resident launches of `ctx` since the last reset as their first block saw them: how many completed, and their summed
 * run time on the device's constant 100 MHz clock (read at the block's first and last instruction).  A cross-check of
 * pf_timing.persist_ms, whose HIP event pairs also contain the dispatch of the kernel and the event packets themselves
 * (~20 us per launch).  Synchronises the ctx stream. */
int pf_persist_clock(pf_ctx* ctx, double* kernel_ms, int64_t* launches, int reset);
/* What the resident path is doing, for callers that want to know whether they are on the fast path. */
typedef struct pf_persist_info {
    int32_t enabled;           /* 1: filter applications use the resident kernels where a graph allows it             */
    int32_t two_step;          /* the pf_persist_two_step level: 0 or 1 (single-graph recurrences)                    */
    int32_t owner;             /* 1: `ctx` owns the path, 0: no ctx has used it yet, -1: another ctx of the process  */
    int32_t timeouts;          /* waits that ran out since the process started (each reported as PF_E_PERSIST_TIMEOUT) */
    int64_t launches;          /* resident launches of this process                                                   */
    int64_t launches_two_step; /* ... of them with two steps per exchange                                             */
    int32_t suspended_for;     /* > 0: a wait ran out; this many filter applications still run one step per launch
                                  before the resident path is tried again (64 after the first timeout, doubled by every
                                  further one; environment PF_PERSIST_REARM = the base, 0 = never again)              */
    int32_t rearms;            /* suspensions that have ended                                                         */
    int32_t owner_switches;    /* times the path moved from one ctx to another (the previous owner's launches had
                                  completed; while they are in flight the other ctx runs one step per launch)         */
    int32_t hold_ticks;        /* the hold-back of the latest resident launch, 10 ns ticks after a step began (0: fixed sleep) */
} pf_persist_info;
int pf_persist_state(pf_ctx* ctx /* nullable */, pf_persist_info* out);
/* The per-graph window structures the resident kernels run on, for tests and diagnostics (read-only; no kernel of its own;
 * no result of any solve changes).  Prepares the first-ring structures if the graph has not yet (and, with want_rings, the
 * second-ring structures too - at once instead of at the graph's third single application), then reports
 *   win_rows, n_windows   rows per window (1024 / 2048 / 4096) and n_pad / win_rows;
 *   state                 1: covered by the resident kernel, 0: not (more than 256 windows, no stored entry, a window with
 *                         more than 4096 outside entries or more than 1024 distinct outside rows);
 *   state2                1: two steps per exchange possible, 0: not (windows of more than 1024 rows, a window with more
 *                         than 512 outside rows or more than 1024 in both rings, an outside row in a SELL slice wider
 *                         than 16, windows that do not hold each other's rows symmetrically), -1: not asked for yet;
 *   ghosts[n_windows]     outside rows each window reads (one-way repairs included)   - written only if state == 1;
 *   need[n_windows]       leading rows each window publishes (one download)           - written only if state == 1;
 *   ghosts2[n_windows]    second-ring rows of each window                            - written only if state2 == 1.
 * The three arrays may be NULL. */
int pf_graph_window_info(pf_graph* g, int32_t want_rings, int32_t* win_rows, int32_t* n_windows, int32_t* state,
                         int32_t* state2, int32_t* ghosts /* nullable */, int32_t* ghosts2 /* nullable */,
                         int32_t* need /* nullable */);
/* Test hook: the next n resident launches start with their abort flag raised (they give up at once and the
 * PF_E_PERSIST_TIMEOUT recovery runs).  Never needed in production. */
int pf_persist_test_hook(int n_launches);
int pf_cheb(pf_graph* g, int32_t op, int32_t src, int32_t dst, int32_t degree, double c, double e, double rho);
/* Two independent recurrences (graphs a and b of one ctx) advanced in lockstep: step k of both in
 * ONE launch while both have steps left, the longer one alone afterwards.  Resident: one launch for the pair where both
 * graphs are covered and fit together; a launch per graph where they are covered but have no joint kernel (windows of
 * 2048+ rows); with a graph that is not covered (pf_graph_window_info: state 0) the pair streams as a pair. */
int pf_cheb2(pf_graph* ga, int32_t op_a, int32_t src_a, int32_t dst_a, int32_t degree_a, double c_a, double e_a, double rho_a,
             pf_graph* gb, int32_t op_b, int32_t src_b, int32_t dst_b, int32_t degree_b, double c_b, double e_b, double rho_b);
int pf_dots(pf_graph* g, int32_t w, int32_t first, int32_t count, double* out);  /* out[b] = <slot first+b, slot w> */
/* classical Gram-Schmidt of slot w against slots [first, first+count), a second pass when the first one cancelled
 * digits: h[count] = summed coefficients, *nrm = ||w|| afterwards (w is left un-normalised). */
int pf_orth(pf_graph* g, int32_t w, int32_t first, int32_t count, double* h, double* nrm);
/* The same in two phases, so that the host can queue the next filter application before it reads the
 * coefficients: begin enqueues the kernels (and, if `normalize`, w <- w/||w|| with the norm taken on the
 * device) plus an asynchronous copy of the results; end waits for them.  One orth in flight per graph. */
int pf_orth_begin(pf_graph* g, int32_t w, int32_t first, int32_t count, int32_t normalize);
int pf_orth_end(pf_graph* g, double* h, double* nrm);
/* pf_orth_begin for the two graphs of a pair (one ctx) in shared launches, as pf_cheb2 does for the filter; each
 * graph's coefficients are collected with its own pf_orth_end. */
int pf_orth_begin2(pf_graph* ga, int32_t w_a, int32_t first_a, int32_t count_a, int32_t normalize_a, pf_graph* gb, int32_t w_b,
                   int32_t first_b, int32_t count_b, int32_t normalize_b);
/* pf_orth_begin2 and, queued right behind it, pf_cheb2 in one call (one outer step of a pipelined pair driver: the device
 * does not wait for the host between the two).  orth[8] = {w, first, count, normalize} of a, then of b; cheb_i[8] =
 * {op, src, dst, degree} of a, then of b; cheb_d[6] = {c, e, rho} of a, then of b. */
int pf_orth_cheb2(pf_graph* ga, pf_graph* gb, const int32_t* orth, const int32_t* cheb_i, const double* cheb_d);
/* 1 (2: see pf_orth_device_passes) if the last pf_orth_end found that the first Gram-Schmidt pass had cancelled digits (|w'| < 0.3 |w|) and ran the
 * second pass itself, after everything queued behind pf_orth_begin: work queued in between that READ slot w (the next
 * filter application of a pipelined driver) saw the un-refined, un-normalised vector and has to be repeated.  Rare:
 * never on the 250k blobs, a few times per solve right after a restart on small graphs. */
int pf_orth_redone(pf_graph* g);
/* on != 0: the second Gram-Schmidt pass runs whenever |w'| < 0.71 |w| (the classical constant) instead of 0.3 |w|: for
 * iterations that come close to exhausting a small space (unfiltered solves of tiny graphs), where the loose criterion
 * loses orthogonality.  on = 2: EVERY step takes the second pass (the full steps of Lanczos with partial
 * reorthogonalisation: one pass against a basis that is orthogonal to 1e-9 only would leave the new vector at that level).
 * Per graph; off by default. */
int pf_orth_strict(pf_graph* g, int32_t on);
/* on != 0: pf_orth_begin / pf_orth_begin2 / pf_orth_cheb2 queue the second pass together with the first; it runs on the
 * device's own verdict (two launches that return at once when the first pass was fine) and reports h1 + h2 itself, so
 * work queued behind the step never reads a stale w: pf_orth_redone then returns 2 ("two passes, nothing to repeat")
 * instead of 1.  For iterations whose steps often cancel digits - restarted Arnoldi with strongly amplified outliers in
 * the basis (asymmetric W): a repeated filter application costs more than the ~5 us of the two idle launches.  Per graph;
 * off by default. */
int pf_orth_device_passes(pf_graph* g, int32_t on);
/* The NEXT pf_orth_begin / pf_orth_begin2 / pf_orth_cheb2 step of this graph - and only that one - takes its basis from TWO
 * ranges of slots: [first, first + split) and [first2, first2 + count - split), with `first` and `count` as passed to that
 * call; the coefficients come back in that order.  For Lanczos with partial reorthogonalisation (pf_eigs_smallest on
 * symmetric W): most steps orthogonalise against the locked null vectors and the last two basis vectors only. */
int pf_orth_split(pf_graph* g, int32_t first2, int32_t split);
/* Process-wide: the LOCAL Gram-Schmidt steps (four vectors at most, one pass: Lanczos with partial reorthogonalisation) as
 * ONE launch (k_orth_local: the blocks of a graph meet at a counter between the dot products and the projection) where
 * the device holds the whole grid at once and the resident path is trusted (pf_persist_state).  0: dot products and
 * projection as two launches, like every other step; 1 / -1: one launch (the default; PF_ORTH_LOCAL=0 in the
 * environment switches it off for the whole process).  The results are bit-identical either way. */
int pf_orth_one_launch(int32_t on);
int pf_scale(pf_graph* g, int32_t slot, double alpha);
/* slots [dst_first, dst_first+k) = slots [src_first, src_first+m) * Y, Y row-major m x k; ranges must not overlap */
int pf_combine(pf_graph* g, int32_t src_first, int32_t m, const double* Y, int32_t k, int32_t dst_first);
int pf_resnorm(pf_graph* g, int32_t ax, int32_t x, double lam, double* out);     /* ||ax - lam x||_2 */
/* the batched forms the Rayleigh-Ritz step uses (one copy and one synchronisation instead of one per vector):
 * out[i][j] = <slot first_a+i, slot first_b+j> (count_a x count_b, row-major); out[i] = ||slot ax_first+i - lam[i] slot x_first+i||_2 */
int pf_gram(pf_graph* g, int32_t first_a, int32_t count_a, int32_t first_b, int32_t count_b, double* out);
int pf_resnorms(pf_graph* g, int32_t ax_first, int32_t x_first, const double* lam, int32_t count, double* out);
/* Eigenvector post-processing (graph.py:254-257 + the sign/scale convention): for each of
 * `count` slots from `first`: x <- sqrt(g) .* x if from_sym; scale to unit 2-norm; flip so the
 * largest-|entry| (lowest index on ties) is positive; if minmax: (v - min)/(max - min) - 0.5.
 * out: host n x count row-major (numpy (n, count) C-order). */
int pf_finalize_vectors(pf_graph* g, int32_t first, int32_t count, int32_t from_sym, int32_t minmax,
                        double* out);
/* The same in two halves: _begin queues the kernels and - on the ctx's copy stream, behind an event - the download
 * into `out` (pinned memory from pf_host_alloc: one DMA; a pageable destination is staged in chunks), and returns;
 * the block is resident and usable by pf_final_rows / pf_knn1_graphs / pf_eigsort_costs at once, and later work on the
 * ctx stream overlaps with the download.  _end waits for the download and checks the result (PF_E_STATE for a
 * vanished vector); `out` must not be read before it returns.  No-op when nothing is pending.  pf_graph_free and the
 * next _begin collect a pending download themselves.  Since round 3 the n x count image may be held back: it is queued
 * behind the next long kernel of the ctx (a 1-NN search of >= 32768 queries) or by _end, whichever comes first - beside
 * the small kernels that follow a solve a 10 MB download costs what it would cost in line.  `out` must therefore stay
 * allocated until _end (or pf_graph_free) has returned; pf_host_free of a block that is still owed its image cancels
 * the download.  PF_DOWNLOAD_DEFER=0: queued at once, as before. */
int pf_finalize_vectors_begin(pf_graph* g, int32_t first, int32_t count, int32_t from_sym, int32_t minmax, double* out);
int pf_finalize_vectors_end(pf_graph* g);
/* out[i][c] = block[i][col[c]] * sign[c] (c < count <= the block's column count, sign = +-1): the image on the host of
 * eigsort's sign flips and column moves (eigsort.py:108-122), computed on the device from the resident block and copied
 * like the first download (pinned `out`, copy stream; collected by pf_finalize_vectors_end).  The block stays as it is. */
int pf_final_remap_begin(pf_graph* g, const int32_t* col, const double* sign, int32_t count, double* out);
/* Pinned (page-locked) host memory for results that should arrive by one DMA; independent of any ctx. */
int pf_host_alloc(size_t bytes, void** out);
int pf_host_free(void* p);
/* Before a pinned block is reused without being freed (a caller-side pool): forget any eigenvector download the library
 * still owes to it (held back by pf_finalize_vectors_begin; left behind by a call that failed) and wait for one in flight.
 * pf_host_free does the same before it unmaps the block. */
int pf_host_detach(void* p);
/* The block written by the last pf_finalize_vectors stays resident in HBM.  out[t][c] = that block's row rows[t]
 * (n_rows x count, row-major): the sampled eigenvector rows of Graph.get_rand_eig_vecs (graph.py:266-267) without
 * touching the host copy. */
int pf_final_rows(pf_graph* g, const int64_t* rows, int64_t n_rows, double* out);
/* the same for the mesh's points (graphs built from a mesh keep them): out[t] = pts[rows[t]] (n_rows x 3), the gather
 * inside Graph.get_rand_normalized_points (graph.py:269-272) */
int pf_point_rows(pf_graph* g, const int64_t* rows, int64_t n_rows, double* out);
/* y = A x on host vectors (tests / roofline probes) */
int pf_spmv_host(pf_graph* g, int32_t op, const double* x, double* y);
/* Repeated mean filter out = (D+I)^-1 (W+I) applied `iterations` times to values[n][ncols]
 * (row-major), graph.py:320-354. */
int pf_mean_filter(pf_graph* g, const double* values, int32_t ncols, int32_t iterations, double* out);

/* ---- nearest neighbour (replaces scipy KDTree(ref).query(qry), k=1, p=2) ------------------ */
/* focusr.py:351-353 (spectral coordinates, d = n_spectral_features) and eigsort.py:203-204
 * (d = 3); d <= 16.  Exact search (uniform-grid pruning, result identical to exhaustive search): squared
 * distance accumulated left to right over the d
 * coordinates without FMA contraction, lowest reference index wins ties.
 * ref: n_ref x d, qry: n_qry x d row-major float64; idx_out[n_qry] int64; d2_out nullable. */
int pf_knn1(pf_ctx* ctx, const double* ref, int64_t n_ref, const double* qry, int64_t n_qry, int32_t d,
            int64_t* idx_out, double* d2_out);
/* How k = 1 searches prune (the results are the same bits either way).  0 (default): by depth - d <= 6 through a grid
 * over the references' two widest axes (pf_knn.hip), d >= 7 through a hierarchy of bounding boxes over ALL d coordinates
 * (pf_knn_tree.hip: leaves of 64 Morton-ordered points, supers of 64 leaves; what keeps deep, poorly aligned embeddings
 * - BASELINE config C5, 1M x 1M, d = 10 - from degenerating into a brute force inside a 2-D rectangle); 1: always the
 * grid; 2: always the hierarchy. */
int pf_knn_mode(pf_ctx* ctx, int32_t mode);
/* Visits of the last hierarchy search, summed over the waves (counted only while enable_counting was 1 for that search;
 * the call also sets the switch for the searches to come). */
int pf_knn_tree_stats(pf_ctx* ctx, int32_t enable_counting, int64_t* leaves_scanned, int64_t* supers_opened);
/* The same for the grid search (k = 1, d <= 9): candidate-query pairs whose squared distance the last counted search
 * evaluated (3 d floating-point operations each): the work behind the 1-NN stage's roofline entry in bench.py. */
int pf_knn_count(pf_ctx* ctx, int32_t enable_counting, int64_t* pairs);
/* Diagnostics of the last COUNTED grid search: the waves' own run times - their sum and the slowest wave, in us - the
 * number of waves, the candidates of the wave that scanned most, and detail[5]: chunks, scans, scan us, bounds us and
 * candidates that pass the off-plane coordinates, summed over the waves. */
int pf_knn_wave_stats(pf_ctx* ctx, double* sum_us, double* max_us, int64_t* waves, int64_t* max_candidates, double* detail);
/* k nearest neighbours (1 <= k <= 4, d <= 4), ascending by (distance, index): the 3-NN of
 * Focusr.get_weighted_final_node_locations (focusr.py:409-412).  idx_out / d2_out: n_qry x k row-major. */
int pf_knn(pf_ctx* ctx, const double* ref, int64_t n_ref, const double* qry, int64_t n_qry, int32_t d, int32_t k,
           int64_t* idx_out, double* d2_out);
/* k nearest neighbours for 1 <= k <= 64 (k <= n_ref) in 1 <= d <= 128 coordinates; n_ref and n_qry in 1 .. 2^31 - 1.
 * d2(q, r) is the sum over the coordinates, from coordinate 0 on, of (q_c - r_c)^2 with separate multiply and add.  Per
 * query: the k references with the smallest (d2, index), ascending - equal distances go to the lower index.  idx_out and
 * d2_out (nullable) are n_qry x k row-major; indices and distances are the bits of a brute force, and two calls give
 * the same bits.  A query with a NaN coordinate compares with nothing: its row is k times (0x7fffffff, +inf), pf_knn's
 * rule.  Non-finite reference coordinates: unspecified result, no fault.  Outside the limits, or with a NULL pointer
 * (d2_out excepted): PF_E_ARG, nothing is launched and the ctx stays usable.
 * d <= 16: a list of the k best per query on the box hierarchy of pf_knn_tree.hip, which then takes n_ref <= 2^31 - 64
 * as it does for pf_knn1; beyond: the same list over an exhaustive scan.  pf_knn (k <= 4, d <= 4) and pf_knn1_wide are
 * unchanged.  pf_timing_get's knn_ms is the device time of the last call, transfers excluded. */
int pf_knn_topk(pf_ctx* ctx, const double* ref, int64_t n_ref, const double* qry, int64_t n_qry, int32_t d, int32_t k,
                int64_t* idx_out, double* d2_out);
/* focusr.py:351-353 with the coordinates taken from the two graphs' resident pf_finalize_vectors blocks instead of
 * host arrays: ref[i][c] = final_ref[i][col_ref[c]] * scale_ref[c], qry likewise (c < d) - the column selection, sign
 * flips and permutation of eigsort (eigsort.py:108-122) and the spectral weights (focusr.py:481-501) are folded into
 * col / scale, so the n x k coordinates never cross PCIe.  Same search, same arithmetic as pf_knn1. */
int pf_knn1_graphs(pf_graph* ref_g, pf_graph* qry_g, int32_t d, const int32_t* col_ref, const double* scale_ref,
                   const int32_t* col_qry, const double* scale_qry, int64_t* idx_out, double* d2_out);
/* The same on any two row-major blocks in device memory (row strides in doubles): what the ranks of a split pair hold
 * after the RCCL all-gather of their resident blocks - qry_block may point at a row range of a block, the
 * query shard of this rank.  The pointers must be valid on ctx's device; work is enqueued on ctx's stream. */
int pf_knn1_blocks(pf_ctx* ctx, const double* ref_block, int64_t n_ref, int32_t ref_stride, const double* qry_block,
                   int64_t n_qry, int32_t qry_stride, int32_t d, const int32_t* col_ref, const double* scale_ref,
                   const int32_t* col_qry, const double* scale_qry, int64_t* idx_out, double* d2_out);
/* eigsort's cost matrices (eigsort.py:162-233) from the graphs' device-resident eigenvector blocks and point copies:
 * m_t / m_s <= 16384 sampled rows of the target / source graph (rows_t / rows_s), the first k eigenmaps of each as
 * final[:, col[c]] * sign[c] (the column permutation and sign flips earlier eigsort calls left, identity at first).
 * out[4][k][k] = c_hist, c_hist_f, c_spatial, c_spatial_f (row = target map, column = source map); idx_out[m_t] = the
 * sampled source point nearest to each sampled target point (min-max normalised xyz, eigsort.py:203-204).
 * A sample without extent along an axis (a planar mesh, one sampled row) normalises to NaN there: idx_out is then
 * 0x7fffffff throughout (pf_knn1's answer for a query nothing compares with) and c_spatial / c_spatial_f are NaN. */
int pf_eigsort_costs(pf_graph* g_target, pf_graph* g_source, const int64_t* rows_t, int64_t m_t, const int64_t* rows_s, int64_t m_s,
                     int32_t k, const int32_t* col_t, const double* sign_t, const int32_t* col_s, const double* sign_s, double* out,
                     int64_t* idx_out);
/* Device address and shape of the resident block ([n_rows][n_cols] row-major float64, owned by the graph, valid until
 * the next pf_finalize_vectors on it or pf_graph_free): lets a peer library (RCCL through torch) send it without a
 * host round trip. */
int pf_final_device(pf_graph* g, double** block, int64_t* n_rows, int32_t* n_cols);
/* split form (inputs resident in HBM across the timed region) */
int pf_knn_upload(pf_ctx* ctx, const double* ref, int64_t n_ref, const double* qry, int64_t n_qry, int32_t d);
int pf_knn_run(pf_ctx* ctx);
int pf_knn_download(pf_ctx* ctx, int64_t* idx_out, double* d2_out);

/* ---- functional maps and ZoomOut (pf_fmap.hip; the reference has none: an extra) --------------------------------
 * Exact 1-NN for 1 <= d <= 128 by a register- and LDS-tiled exhaustive scan: pf_knn1's arithmetic (left to right,
 * separate multiply and add, lowest reference index on exact ties), so indices and distances are a brute force's bits.
 * For d <= 16 pf_knn1 stays the production path (it prunes); this one takes small d so that the two can be compared.
 * Non-finite coordinates: unspecified winner (no fault).  PF_E_ARG for d outside 1..128 or an empty set. */
int pf_knn1_wide(pf_ctx* ctx, const double* ref, int64_t n_ref, const double* qry, int64_t n_qry, int32_t d,
                 int64_t* idx_out, double* d2_out /* nullable */);
/* Coordinate pairs ((q_c - r_c)^2 terms, 3 floating-point operations each, padding to chunks of 8 coordinates and 16
 * references included) that the last COUNTED wide search evaluated - a wave drops 16 references once none of their
 * partial sums is below its lanes' best; the call also sets the switch for the searches to come. */
int pf_knn1_wide_count(pf_ctx* ctx, int32_t enable_counting, int64_t* coordinate_pairs);
/* A point map T (T[i] in [0, n_t) for every SOURCE vertex i: Focusr's direction) and two M-orthonormal Laplace-Beltrami
 * bases, ascending (laplace_beltrami_spectrum), resident for the whole iteration:
 *   project  C[a][b] = sum_i mass_s[i] phi_s[i][a] phi_t[T[i]][b], k_s x k_t row-major: the coefficients of a function
 *            on the target -> those of its pull-back on the source.  Rows in blocks of 512, each block summed in row
 *            order, the blocks added in block order; no floating-point atomics: two calls give the same bits.
 *   convert  Q = phi_s[:, :k_s] C (every entry summed over a ascending), then T[i] = the row of phi_t[:, :k_t] nearest
 *            to Q[i]: the library's search for k_t <= 16, the wide scan above it; exact, lowest index on ties.
 *   zoomout  k = k_start; loop { project (k, k); convert (k, k); stop at k == k_end; k = min(k + step, k_end) }, then
 *            n_iter_at_end more rounds at k_end.  C_out (nullable): the last projection, k_end x k_end.
 * pf_fmap_create      phi_t [n_t][K], phi_s [n_s][K], mass_s [n_s] (host), 1 <= K <= 128.
 * pf_fmap_set_p2p     T [n_s]; validated on the device: an entry outside 0 .. n_t - 1 gives PF_E_ARG (no map is set).
 * pf_fmap_get_p2p     T_out [n_s]; d2_out [n_s] (nullable) the squared distances of the last convert (PF_E_STATE if none).
 * pf_fmap_project     1 <= k_s, k_t <= K; C_out nullable; C stays resident.  PF_E_STATE without a point map.
 * pf_fmap_convert     C (host, k_s x k_t) or NULL for the resident one (PF_E_STATE if its shape differs).
 * Everything runs on the ctx stream. */
typedef struct pf_fmap pf_fmap;
int pf_fmap_create(pf_ctx* ctx, const double* phi_t, int64_t n_t, const double* phi_s, int64_t n_s, const double* mass_s,
                   int32_t K, pf_fmap** out);
void pf_fmap_free(pf_fmap* h);
int pf_fmap_set_p2p(pf_fmap* h, const int64_t* T);
int pf_fmap_get_p2p(pf_fmap* h, int64_t* T_out, double* d2_out);
int pf_fmap_project(pf_fmap* h, int32_t k_s, int32_t k_t, double* C_out);
int pf_fmap_convert(pf_fmap* h, const double* C, int32_t k_s, int32_t k_t);
int pf_fmap_zoomout(pf_fmap* h, int32_t k_start, int32_t k_end, int32_t step, int32_t n_iter_at_end, double* C_out);
/* ZoomOut on sub-samples (Melzi et al. 2019, 4.2.3).  A = phi_s[S_s] (q_s rows), B = phi_t[S_t] (q_t rows), gathered once:
 *   k = k_start;  C = project (k, k) of the handle's full point map;
 *   loop { Tsub[i] = the row of B[:, :k] nearest to (A[:, :k] C)[i];  last = (k == k_end and the n_iter_at_end extra rounds
 *          are used up);  k = min(k + step, k_end);  C = the least-squares fit on the samples at the new k, the solution of
 *          (A_k^T A_k) C = A_k^T B[Tsub, :k];  stop if last }
 *   convert (k_end, k_end) at full resolution: the handle's point map and distances are the full ones.
 * Both Gram products are summed on the device in project's fixed order (two calls give the same bits); the k x k system
 * is solved on the host by a Cholesky factorisation: one wait per round for k_end^2 doubles.
 * pf_fmap_set_samples     indices into the target and the source (host), q_t, q_s >= 1; validated on the device: an entry
 *                         out of range gives PF_E_ARG (no samples are set).
 * pf_fmap_zoomout_sampled PF_E_STATE without samples or a point map; PF_E_ARG unless q_s >= k_end; PF_E_DEGENERATE when a pivot
 *                         of the factorisation is not positive beyond its rounding, (q_s + k) eps times the diagonal
 *                         entry (the samples are too few or degenerate for this k).
 *                         C_out (nullable): the last fit, k_end x k_end. */
int pf_fmap_set_samples(pf_fmap* h, const int64_t* S_t, int64_t q_t, const int64_t* S_s, int64_t q_s);
int pf_fmap_zoomout_sampled(pf_fmap* h, int32_t k_start, int32_t k_end, int32_t step, int32_t n_iter_at_end, double* C_out);

/* ---- farthest-point sampling (pf_fps.hip; the reference has none: an extra) ----------------------------------------
 * m samples of the n x d points (host, row-major, 1 <= d <= 16, 1 <= m <= n < 2^31).  d2(i, c) = the sum over the
 * coordinates, left to right, of (P[i][x] - c[x])^2, separate multiply and add.  start >= 0: the first sample; -1: the
 * point with the largest d2 to the centroid (the per-coordinate mean, summed in index order), lowest index on ties.
 * dmin = +inf, owner = 0; round j: sel[j] = cur; every i with d2(i, cur) < dmin[i] takes dmin[i] = d2(i, cur), owner[i] = j;
 * cur = argmax dmin, lowest index on ties.  Samples repeat (index 0) once m exceeds the number of distinct points.
 * sel_out [m]; owner_out [n] (nullable) the position in sel of the nearest sample, the earliest on ties; dmin_out [n]
 * (nullable) the squared distance to it: its maximum is the squared covering radius.  2 m launches back to back, one
 * download.  PF_E_ARG for d, m or start out of range or a coordinate that is not finite. */
int pf_fps(pf_ctx* ctx, const double* points, int64_t n, int32_t d, int64_t m, int64_t start, int64_t* sel_out,
           int32_t* owner_out, double* dmin_out);

/* ---- spectral descriptors (pf_descriptors.hip; the reference has none: an extra) ---------------------------------
 * Every descriptor sum_a phi[i][a]^2 g_t(lambda_a) - heat kernel signature, wave kernel signature, ... - through one
 * host-made table G [K][T] row-major (K basis functions, T samples).  All arrays are host arrays, FP64, row-major; no
 * handle, no state; everything runs on the ctx stream and the call returns when the result has arrived.
 *   pf_spectral_descriptors     out[i][t] = sum_a (phi[i][a] * phi[i][a]) * G[a][t], n x T: a ascending, a separate
 *            multiply and a separate add per term (no contraction): the bits of the plain loop.
 *   pf_descriptor_coefficients  A_out[a][t] = sum_i phi[i][a] * (mass[i] * F[i][t]), k_out x T, a < k_out <= K, with F
 *            the array above (all K columns of phi enter it), formed on chip and never written to memory.  Rows in
 *            blocks of 512, each block summed in row order, the blocks added in block order; no floating-point
 *            atomics: two calls give the same bits.  A row with mass 0 or with phi all zero adds exactly 0.
 * Limits: n >= 1, 1 <= K <= 128, 1 <= T <= 512, 1 <= k_out <= K; outside them, or with a NULL pointer, PF_E_ARG and
 * nothing is launched.  PF_E_HIP for a failed allocation, copy or launch. */
int pf_spectral_descriptors(pf_ctx* ctx, const double* phi, int64_t n, int32_t K, const double* G, int32_t T, double* out);
int pf_descriptor_coefficients(pf_ctx* ctx, const double* phi, const double* mass, int64_t n, int32_t K, const double* G,
                               int32_t T, int32_t k_out, double* A_out);

/* ---- the whole eigensolve in one call --------------------------------------------------------------------------
 * Replaces scipy.sparse.linalg.eigs(L, k, sigma=1e-10, which="LM", ncv=4k) at graph.py:372 (called from
 * recursive_eig, graph.py:357-389) for callers that bind the C-ABI without the Python driver: the n_wanted lowest
 * eigenpairs with eigenvalue > 1e-10 (graph.py:381) of the graph's random-walk Laplacian, ascending; vecs is
 * [n][*n_out] row-major, unit 2-norm, sign fixed (largest-|entry| positive), min-max normalised to [-0.5, 0.5] when
 * minmax != 0 (graph.py:254-257).  The reference's widen-and-retry rule (graph.py:369-384) only changes HOW MANY pairs
 * it asks for: a caller that wants its column count asks for k_final - #nulls, with #nulls = n_components +
 * n_isolated of pf_graph_get_info.  Symmetric W: thick-restart Lanczos on S = G^1/2 (D - W) G^1/2.  Asymmetric W
 * (one-way edges, graph.py:178: both bundled 15k meshes): restarted Arnoldi on L itself - the complex eigenvalues of
 * the non-normal L are carried as dominant Ritz values of the interval filter, or, when the low eigenvalues are complex
 * themselves (open surfaces), enclosed by the ellipse filter; real parts are returned as the reference does
 * (graph.py:386-389), a conjugate pair as a repeated value with a fixed phase.  Graphs of fewer than ~100 vertices and
 * operators whose wanted eigenvalues are no corner of the spectrum are refused with PF_E_STATE (pyfocusr_amd/_krylov.py
 * keeps the unfiltered mode for them).  vals needs room for n_wanted values, vecs for n * n_wanted. */
typedef struct pf_eigs_stats {
    int64_t matvecs;      /* SpMV-equivalent launches */
    int32_t outer_steps;  /* Lanczos steps */
    int32_t restarts;
    int32_t filter_resets;
    int32_t degree;       /* of the last Chebyshev filter */
    int32_t n_null;       /* eigenvalues <= 1e-10 found among the computed ones (= locked null vectors) */
    double cut;           /* lower end of the damped interval */
    double max_residual;  /* max ||S x - lambda x||_2 of the returned pairs */
    int32_t second_passes; /* outer steps whose Gram-Schmidt projection cancelled digits (second pass run) */
    int32_t mode;          /* 0: symmetric W (Lanczos on S); 1: asymmetric W, interval filter (Arnoldi on L, complex outliers carried); 2: ellipse filter */
    int32_t local_steps;   /* symmetric W: outer steps that orthogonalised against the null vectors and the last two basis vectors only
                              (partial reorthogonalisation; the others were full Gram-Schmidt steps) */
    int32_t reserved;
} pf_eigs_stats;
int pf_eigs_smallest(pf_graph* g, int32_t n_wanted, int32_t minmax, double* vals, double* vecs, int32_t* n_out,
                     pf_eigs_stats* stats);
/* The same with the options of the pair call: residuals (nullable) = ||A x - lambda x||_2 per returned pair;
 * async_download = 1: the call returns with the eigenvector download still in flight into vecs (pinned: pf_host_alloc) -
 * pf_finalize_vectors_end(g) before reading it. */
int pf_eigs_smallest_ex(pf_graph* g, int32_t n_wanted, int32_t minmax, int32_t async_download, double* vals, double* vecs,
                        double* residuals, int32_t* n_out, pf_eigs_stats* stats);
/* The two graphs of a pair (target and source mesh of focusr.py:134-170; one ctx; symmetric or not, each by its own) solved TOGETHER: the
 * two iterations advance in lockstep, every Gram-Schmidt step and filter application that both have pending runs in
 * launches the graphs share (pf_orth_cheb2: one library call and three launches per outer step of the pair), one graph
 * finishes alone once its partner has converged.  res_a / res_b (nullable): ||S x - lambda x||_2 per returned pair.
 * async_download = 1: the call returns with the eigenvector downloads still in flight (pf_finalize_vectors_begin into
 * vecs_a / vecs_b, which should be pinned: pf_host_alloc) - pf_finalize_vectors_end(g) before reading them; the
 * device-resident blocks are usable at once.  vals need room for n_wanted values, vecs for n * n_wanted; when a graph
 * returns fewer pairs (*n_out < n_wanted) its vecs hold an n x *n_out block. */
int pf_eigs_smallest2(pf_graph* ga, pf_graph* gb, int32_t n_wanted_a, int32_t n_wanted_b, int32_t minmax, int32_t async_download,
                      double* vals_a, double* vecs_a, double* res_a, int32_t* n_out_a, pf_eigs_stats* stats_a,
                      double* vals_b, double* vecs_b, double* res_b, int32_t* n_out_b, pf_eigs_stats* stats_b);

/* ---- primitives of the row-partitioned solve (one large mesh over several GPUs; SURVEY 8e / BASELINE config C5).
 * The reference has no counterpart (scipy eigs on one core, graph.py:357-389).  pyfocusr_amd/rowpart.py drives them.
 *   pf_op_step     one step of a three-term recurrence: out = alpha (shift x - A x) - beta prev   (slots; prev = -1:
 *                  no prev term; out may be the prev slot)
 *   pf_cheb_steps  steps k_first .. k_first+n_steps-1 of the Chebyshev recurrence of pf_cheb on explicit state: slot
 *                  `cur` holds y_{k_first-1}, slot `prev` holds y_{k_first-2} (ignored and overwritten when
 *                  k_first = 1); each step writes y_k over y_{k-2}; *out_cur / *out_prev tell where y_last and
 *                  y_{last-1} ended up
 *   pf_axpy        slot w += sum_i coef[i] * slot (first + i)
 *   pf_rows_*      a fixed subset of rows (mesh-order indices): gather its values of a slot to the host, scatter
 *                  host values into it, or fill it with a constant — the boundary / ghost rows of a partition. */
typedef struct pf_rows pf_rows;
int pf_op_step(pf_graph* g, int32_t op, int32_t x, int32_t prev, int32_t out, double alpha, double shift, double beta);
int pf_cheb_steps(pf_graph* g, int32_t op, int32_t prev, int32_t cur, int32_t k_first, int32_t n_steps, double c, double e,
                  double rho, int32_t* out_prev, int32_t* out_cur);
int pf_axpy(pf_graph* g, int32_t w, int32_t first, int32_t count, const double* coef);
int pf_rows_create(pf_graph* g, const int64_t* rows, int64_t n, pf_rows** out);
void pf_rows_free(pf_rows* r);
int pf_rows_gather(pf_rows* r, int32_t slot, double* out);
int pf_rows_scatter(pf_rows* r, int32_t slot, const double* in);
int pf_rows_gather_dev(pf_rows* r, int32_t slot, double* dst_device);        /* device buffers of the caller (e.g. a */
int pf_rows_scatter_dev(pf_rows* r, int32_t slot, const double* src_device); /* tensor RCCL sends / received); no sync */
/* one launch each way for BOTH vectors of a boundary exchange: dst[t] = slot_a[row t], dst[stride + t] = slot_b[row t]
 * (slot_b = -1: only a);  slot_a[row t] = src[off t], slot_b[row t] = src[off t + stride] with the per-row offsets
 * of pf_rows_set_sources (where each ghost row's value sits in the all-gathered receive buffer) */
int pf_rows_set_sources(pf_rows* r, const int64_t* offsets);
int pf_rows_gather2_dev(pf_rows* r, int32_t slot_a, int32_t slot_b, double* dst_device, int64_t stride);
int pf_rows_scatter2_dev(pf_rows* r, int32_t slot_a, int32_t slot_b, const double* src_device, int64_t stride);
int pf_rows_fill(pf_rows* r, int32_t slot, double value);

/* ---- closest point on a triangulated surface (ICP pre-alignment, "next" row f3) --------------------------
 * Replaces the vtkCellLocator::FindClosestPoint loop inside vtkIterativeClosestPointTransform, which the
 * reference runs through vtk_functions.py:12-29 (called from focusr.py:110-131).  Polygons with more than three
 * vertices are fan-triangulated (0,j+1,j+2).  Exact: the minimum over all triangles of the exact point-triangle
 * distance; lowest face index on exact ties.
 *   pf_surface_create   points [n][3] f64, faces [n_faces][verts_per_face] i32 (host) -> device search structure
 *   pf_surface_closest  qry [n_qry][3] f64 (host) -> out_pts [n_qry][3] closest surface points, out_face [n_qry]
 *                       face index (-1 and NaN point for a NaN query), out_d2 [n_qry] squared distances; each
 *                       output may be NULL. */
typedef struct pf_surface pf_surface;
int pf_surface_create(pf_ctx* ctx, const double* points, int64_t n, const int32_t* faces, int64_t n_faces,
                      int32_t verts_per_face, pf_surface** out);
void pf_surface_free(pf_surface* s);
int pf_surface_closest(pf_surface* s, const double* qry, int64_t n_qry, double* out_pts, int32_t* out_face,
                       double* out_d2);
/* Surface distances of many queries (whole meshes: every vertex of one mesh against the surface of another).  Same
 * exact minimum and tie rule as pf_surface_closest, so out_d2 and out_face equal its outputs bit for bit; no closest
 * points.  The queries are Morton-sorted on the device and searched in packets of 16 neighbours (4 for fewer than
 * 65536 queries), each chunk of triangles loaded once per packet.
 *   pf_surface_distance  qry [n_qry][3] f64 (host), n_qry >= 1 (else PF_E_ARG) -> out_d2 [n_qry] exact squared
 *                        distances, out_face [n_qry] face index (a query with a non-finite coordinate: NaN and -1);
 *                        stats [6] = n_finite | n_nan | sum d | sum d^2 | max d | argmax (as double; -1 if none) over
 *                        the queries with a finite d = sqrt(d2), n_nan counting the others, argmax the lowest query
 *                        index of the largest d2; sums in a fixed order (two calls give identical bits).  Each output
 *                        may be NULL. */
int pf_surface_distance(pf_surface* s, const double* qry, int64_t n_qry, double* out_d2, int32_t* out_face,
                        double* stats);
/* Signed surface distances (angle-weighted pseudonormals, Baerentzen & Aanaes 2005).  sd = sign((p - c) . n) sqrt(d2)
 * with c the closest point on the winning triangle and n the pseudonormal of the feature c lies on: the unit face
 * normal (interior; right-hand rule of the face's vertex order), the sum of the unit normals of the edge's triangles
 * (edge; fan diagonals are edges), sum of corner angle x unit normal (vertex).  sd > 0 on the side the face normals
 * point to: on an outward-oriented closed mesh inside is negative.  Sums in a fixed order, no floating-point atomics.
 *   pf_surface_prepare_signed   the host points [n][3] f64 and faces [n_faces][verts_per_face] i32 given to
 *                               pf_surface_create again (that call keeps no copy) -> device copies, face normals, edge and
 *                               vertex pseudonormals; topology [4] (may be NULL) = edges | boundary edges (one triangle) |
 *                               non-manifold edges (three or more) | inconsistent edges (two triangles that traverse it in
 *                               the same direction), counted over the fan triangles' edges.  A second call rebuilds.
 *   pf_surface_signed_distance  qry [n_qry][3] f64 (host), n_qry >= 1 -> out_sd [n_qry] (|sd| = sqrt(out_d2 of
 *                               pf_surface_distance) bit for bit; +0.0 at distance 0; NaN for a non-finite query),
 *                               out_face [n_qry] (= pf_surface_distance's), out_feature [n_qry] 0 face | 1 edge | 2 vertex
 *                               (-1 with face -1), n_ambiguous: queries with d2 > 0 whose (p - c) . n is 0 (e.g. a zero
 *                               pseudonormal of degenerate triangles), returned as +sqrt(d2).  Each output may be NULL.
 *                               PF_E_ARG before pf_surface_prepare_signed. */
int pf_surface_prepare_signed(pf_surface* s, const double* points, const int32_t* faces, int64_t* topology);
int pf_surface_signed_distance(pf_surface* s, const double* qry, int64_t n_qry, double* out_sd, int32_t* out_face,
                               int32_t* out_feature, int64_t* n_ambiguous);
/* Generalized winding numbers (Jacobson et al. 2013; hierarchical evaluation after Barill et al. 2018).
 * w(q) = (1 / 4 pi) sum_t Omega_t(q) over the fan triangles, Omega the signed solid angle (Van Oosterom & Strackee):
 * Omega = 2 atan2(a . (b x c), |a||b||c| + (a . b)|c| + (b . c)|a| + (c . a)|b|) with a, b, c the corners minus q; a
 * triangle with a corner exactly at q gives 0.  w is 1 inside and 0 outside a closed outward-oriented mesh (reversed
 * faces subtract), varies smoothly across holes and needs no normals, edges or manifoldness.  Works on the structure
 * pf_surface_create built (no host arrays again).  Sums in a fixed order, no floating-point atomics: two calls give
 * identical bits.  Against a host evaluation only a tolerance holds (summation order, FMA and atan2 differ).
 *   pf_surface_prepare_winding  per chunk of 64 triangles and per super-chunk of 64 chunks the dipole data: N = sum of
 *                               1/2 (b - a) x (c - a), A = sum of areas, the area-weighted centroid (the box centre if
 *                               A = 0), r = max |corner - centroid|.  A second call does nothing.
 *   pf_surface_winding          qry [n_qry][3] f64 (host), n_qry >= 1 -> out_w [n_qry], out_bound [n_qry]; each may be NULL.
 *                               beta <= 0: every triangle through the exact term; out_bound is 0.  beta > 1: a cluster
 *                               (super-chunk, then chunk) whose centroid is at d >= beta r from every finite query of a
 *                               packet of 8 neighbouring queries contributes N . (p - q) / (4 pi d^3) instead of its
 *                               triangles, and A r / (2 pi (d - r)^3) to out_bound: |out_w - w| <= out_bound up to the
 *                               rounding of the sums.  0 < beta <= 1 (q may lie inside the ball), NaN or +inf: PF_E_ARG.
 *                               A query with a non-finite coordinate gives NaN in both outputs.  PF_E_ARG for n_qry < 1
 *                               or before pf_surface_prepare_winding. */
int pf_surface_prepare_winding(pf_surface* s);
int pf_surface_winding(pf_surface* s, const double* qry, int64_t n_qry, double beta, double* out_w, double* out_bound);
/* Ray casting: first hit, barycentric coordinates and crossing count of many rays o + t d against the fan triangles,
 * on the structure pf_surface_create built.  One exact test in f64 without FMA (Moeller-Trumbore; d is not normalised,
 * so t is in units of |d|):
 *   e1 = b - a, e2 = c - a, p = d x e2, det = e1 . p, tv = o - a, u = (tv . p) / det, q = tv x e1, v = (d . q) / det,
 *   t = (e2 . q) / det;  a triangle is accepted when det != 0, u >= 0, v >= 0, u + v <= 1, t_min <= t <= t_max (both ends
 *   inclusive) and facing allows it: 0 any side, +1 only det > 0 (the ray meets the side the face normal points to),
 *   -1 only det < 0.  NaN triangles never pass; zero-area triangles have det = 0.
 * The result of a ray is that of this test over ALL fan triangles, bit for bit (box pruning only skips triangles the test
 * cannot accept: the argument is in pf_surface.hip).  The test is not watertight: a ray exactly through an edge or a vertex
 * may be accepted by several triangles or by none.
 *   pf_surface_raycast         origins, dirs [n_rays][3] f64 (host), n_rays >= 1 -> out_t [n_rays] the least accepted t
 *                              (ties: lowest fan-triangle index), out_face [n_rays] that triangle's face, out_uv
 *                              [n_rays][2] its (u, v): the hit point is a + u e1 + v e2; out_count [n_rays] the number of
 *                              accepted triangles in [t_min, t_max].  A miss gives +inf, -1, NaN uv, count 0; a ray with a
 *                              non-finite origin or direction component or a zero direction gives NaN, -1, NaN uv, count 0.
 *                              Each output may be NULL; without out_count the search narrows the interval to the best t
 *                              found.  PF_E_ARG for n_rays < 1, NaN t_min / t_max, t_min > t_max, facing outside {-1, 0, 1}.
 *                              The rays are Morton-sorted by origin on the device and traced in packets of 16 neighbours (4
 *                              for fewer than 65536 rays); two calls give identical bits.
 *   pf_surface_vertex_normals  out [n][3]: the angle-weighted vertex pseudonormals (sum of corner angle x unit normal) as
 *                              pf_surface_prepare_signed stored them, not normalised (zero for an unreferenced vertex).
 *                              PF_E_ARG before pf_surface_prepare_signed. */
int pf_surface_raycast(pf_surface* s, const double* origins, const double* dirs, int64_t n_rays, double t_min, double t_max,
                       int32_t facing, double* out_t, int32_t* out_face, double* out_uv, int32_t* out_count);
int pf_surface_vertex_normals(pf_surface* s, double* out);

/* ---- closest point on a surface embedded in d dimensions (sub-vertex correspondences) ---------------------
 * FOCUSR matches a source vertex to the nearest target VERTEX in spectral coordinates (focusr.py:351-353).  The target
 * is a triangulated surface in the same d-dimensional space; this is the closest point ON it: a fan triangle and
 * barycentric weights.  1 <= d <= 16 (the limit of pf_knn_upload and pf_assign).  Polygons are fan-triangulated
 * (0,j+1,j+2).  Exact: the minimum over ALL fan triangles of the exact point-triangle squared distance, lowest
 * fan-triangle index on exact ties; a triangle whose distance is NaN (a degenerate one, through the divisions of the walk)
 * never wins.  The arithmetic is the region walk of pf_surface_closest with every dot product summed left to right over
 * coordinates 0 .. d-1 without FMA, the closest point formed per coordinate by the region's formula and d2 the sum of the
 * squared coordinate differences, left to right: a host loop in the same order gives the same bits, and at d = 3 out_d2
 * and out_face equal pf_surface_closest's.  No floating-point atomics: two calls give identical bits.
 *   pf_surface_nd_create   coords [n][d] f64, faces [n_faces][verts_per_face] i32 (host) -> device search structure.
 *                          PF_E_ARG for d outside 1..16, n < 1, no faces, verts_per_face outside 3..16, a vertex id
 *                          outside 0..n-1.
 *   pf_surface_nd_closest  qry [n_qry][d] f64 (host), n_qry >= 1 (else PF_E_ARG) -> out_face [n_qry] the face of the
 *                          winning fan triangle, out_verts [n_qry][3] its vertex ids in its corner order (a, b, c),
 *                          out_bary [n_qry][3] the weights of the region the walk ended in: (1,0,0) (0,1,0) (0,0,1) at a
 *                          corner, (1-v, v, 0) on ab, (1-w, 0, w) on ca, (0, 1-w, w) on bc, ((1-v)-w, v, w) inside;
 *                          out_d2 [n_qry] the squared distance.  A query with a non-finite coordinate, or a surface
 *                          without a triangle of finite distance, gives -1, (-1,-1,-1), NaN weights, NaN.  Each output
 *                          may be NULL.  exhaustive != 0 tests every triangle against every query (no box pruning): the
 *                          same bits, the device-side yardstick of the pruned search.
 *   pf_surface_nd_last_search  of the last pf_surface_nd_closest on s: chunks of 64 triangles staged, summed over the
 *                          packets of 8 neighbouring queries; the number of packets; the chunks of the surface.  Each
 *                          may be NULL. */
typedef struct pf_surface_nd pf_surface_nd;
int pf_surface_nd_create(pf_ctx* ctx, const double* coords, int64_t n, int32_t d, const int32_t* faces, int64_t n_faces,
                         int32_t verts_per_face, pf_surface_nd** out);
void pf_surface_nd_free(pf_surface_nd* s);
int pf_surface_nd_closest(pf_surface_nd* s, const double* qry, int64_t n_qry, int32_t* out_face, int32_t* out_verts,
                          double* out_bary, double* out_d2, int32_t exhaustive);
int pf_surface_nd_last_search(pf_surface_nd* s, int64_t* chunks_opened, int64_t* packets, int64_t* n_chunks);

/* ---- Coherent Point Drift pieces ("next" row f4) ------------------------------------------------------------
 * The reference registers the spectral coordinates with the third-party cycpd package (focusr.py:297-334).
 * These are the two O(M*N) operations of its EM iteration, matrix-free (P and G are never stored):
 *   pf_cpd_create  X [N][d] fixed set, Y [M][d] moving set (host) -> handle; the moving set's current position
 *                  TY starts as Y.
 *   pf_cpd_estep   TY [M][d] (host; NULL = keep the device copy), sigma2 > 0, outlier weight 0 <= w < 1 ->
 *                  P1 [M] = P 1, Pt1 [N] = P^T 1, PX [M][d] = P X with
 *                  P_mn = exp(-|x_n - ty_m|^2 / 2 sigma2) / (sum_m' exp(..) + (2 pi sigma2)^(d/2) w/(1-w) M/N)
 *                  (a zero column sum is replaced by DBL_EPSILON first).  Outputs may be NULL.
 *   pf_cpd_set_basis / pf_cpd_weighted_gram   Q [M][K] (host) stays on the device; H [K][K] = Q^T diag(P1) Q with
 *                  the P1 of the last pf_cpd_estep: the K x K matrix of the low-rank (Woodbury) deformable M-step.
 *   pf_cpd_gram    out [n_a][n_cols] = G(A,B) V,  G_ij = exp(-|a_i - b_j|^2 / 2 beta^2), V [n_b][n_cols] (all host). */
typedef struct pf_cpd pf_cpd;
int pf_cpd_create(pf_ctx* ctx, const double* X, int64_t N, const double* Y, int64_t M, int32_t d, pf_cpd** out);
void pf_cpd_free(pf_cpd* h);
int pf_cpd_estep(pf_cpd* h, const double* TY, double sigma2, double w, double* P1, double* Pt1, double* PX);
int pf_cpd_set_basis(pf_cpd* h, const double* Q, int32_t K);
int pf_cpd_weighted_gram(pf_cpd* h, double* H);
/* Device-resident EM iterations: after pf_cpd_estep(h, NULL, sigma2, w, NULL, NULL, NULL) the posterior sums stay
 * on the device; only the small moment sums an M-step needs come back, and only the new parameters go in.
 *   pf_cpd_affine_sums   shifts [32] = cx[16] | cy[16] (means of X and Y, the centre the sums are taken about);
 *                        sums [2 d^2 + 3 d + 3], with xc = x - cx, yc = y - cy, PXc_m = PX_m - P1_m cx:
 *                        sum P1 | sum PXc [d] | sum P1 yc [d] | sum PXc yc^T [d][d] | sum P1 yc yc^T [d][d] |
 *                        sum Pt1 | sum Pt1 |xc|^2 | sum Pt1 xc [d]
 *   pf_cpd_apply_affine  TY = Y B + t
 *   pf_cpd_deform_sums   H [K][K] = Q^T diag(P1) Q,  R [K][d] = Q^T (PX - diag(P1) Y)      (needs pf_cpd_set_basis)
 *   pf_cpd_apply_deform  TY = Y + Q C (C [K][d]), then sums [5] = sum P1 | sum P1 |ty|^2 | sum ty.PX | sum Pt1 |
 *                        sum Pt1 |x|^2 with the new TY
 *   pf_cpd_download      current TY [M][d] and the last posterior sums (each may be NULL) */
int pf_cpd_affine_sums(pf_cpd* h, double* shifts, double* sums);
int pf_cpd_apply_affine(pf_cpd* h, const double* B, const double* t);
int pf_cpd_deform_sums(pf_cpd* h, double* H, double* R);
int pf_cpd_apply_deform(pf_cpd* h, const double* C, double* sums);
int pf_cpd_download(pf_cpd* h, double* TY, double* P1, double* Pt1, double* PX);
int pf_cpd_gram(pf_ctx* ctx, const double* A, int64_t n_a, const double* B, int64_t n_b, int32_t d, double beta,
                const double* V, int32_t n_cols, double* out);

/* ---- optimal one-to-one assignment (replaces linear_sum_assignment(cdist(rows, cols)), focusr.py:340-349) ---------- */
/* Exact linear assignment on Euclidean costs C[i][j] = sqrt(sum_c (rows[i][c] - cols[j][c])^2), accumulated left to right
 * without FMA contraction (cdist's `euclidean`); costs are recomputed from the coordinates, no n x n matrix exists.
 * Forward auction with eps-scaling on the problem padded to square by n_cols - n_rows virtual rows of cost 0, candidate
 * lists of each row's 16 nearest columns (a row bids from its list only when the list provably holds its best and
 * second-best column, otherwise it scans every column), then a dense certificate pass:
 *   u_i = min_j (C_ij - v_j) over ALL columns, v_j <= 0 (column prices, shifted), slack_i = C_i,col(i) - u_i - v_col(i) >= 0
 * so that (u, v) is dual-feasible (u_i + v_j <= C_ij) and gap_bound = sum of the slacks (virtual rows included) bounds
 * total_cost - optimum.  The final eps is chosen so that n_cols * eps <= 1e-10 * sum_i min_j C_ij; an eps below
 * 2^-43 * (max C + max price) is not representable and is clamped there (eps_floor_hit; gap_bound then only promises
 * n_cols * eps).  1 <= d <= 16, 1 <= n_rows <= n_cols < 2^31; non-finite coordinates: PF_E_ARG.  Equal costs (duplicate
 * points) may yield another optimal assignment than scipy's.  Deterministic: identical inputs give identical outputs.
 * col_of_row[n_rows]; u_out[n_rows], v_out[n_cols] and stats nullable. */
typedef struct pf_assign_stats {
    int32_t phases;           /* eps-scaling phases run                                                            */
    int32_t dense_passes;     /* certificate passes over all n_rows x n_cols pairs                                  */
    int64_t rounds;           /* Jacobi bid rounds, summed over the phases                                          */
    int64_t bids;             /* bids placed (each row of a round that bid)                                          */
    int64_t dense_bids;       /* ... of them after a scan of all columns (the candidate list could not decide)       */
    int64_t candidate_edges;  /* entries of the candidate lists (n_rows * 16, or n_rows * n_cols when n_cols <= 16)   */
    int64_t launches;         /* kernel launches                                                                      */
    int64_t device_bytes;     /* device memory the call allocated: O(n * (d + 16))                                    */
    int32_t k;                /* candidates per row                                                                   */
    int32_t eps_floor_hit;    /* the final eps was clamped at the float64 floor                                        */
    double eps_initial, eps_final, eps_floor;
    double total_cost;        /* sum of C over the assigned pairs                                                      */
    double gap_bound;         /* proven upper bound of total_cost - optimum (sum of the slacks)                        */
    double lower_bound;       /* sum over the rows of their smallest cost                                              */
    double ms_candidates, ms_auction, ms_certificate;  /* device time of the three stages (HIP events)               */
} pf_assign_stats;
int pf_assign(pf_ctx* ctx, const double* rows, int64_t n_rows, const double* cols, int64_t n_cols, int32_t d,
              int64_t* col_of_row, double* u_out, double* v_out, pf_assign_stats* stats);

/* ---- discrete curvatures of a triangle mesh (the quantities of vtkCurvatures, vtk_functions.py:40-74) --------------
 * pts [n][3] f64, faces [n_faces][3] i32 (host; triangles only).  f64 throughout, separate multiplies and adds, dot
 * products left to right.  Per triangle t = (v0, v1, v2): n_t = (x1 - x0) x (x2 - x0) / |..|, area_t = |..| / 2, corner
 * angle at corner j = atan2(|e1 x e2|, e1 . e2) with e1, e2 the edges that leave the corner; all zero for a zero-area or
 * non-finite triangle.  Half-edge h = 3 t + j leaves corner j of triangle t; every per-vertex sum runs over the
 * half-edges that leave the vertex, in ascending h.
 *   area      A_v = (sum area_t) / 3                                  (barycentric; 0: unreferenced, or only zero-area faces)
 *   gauss     K_v = (2 pi - sum corner angles) / A_v                  (angle defect)
 *   dihedral  of an edge shared by exactly two triangles with non-zero areas that traverse it in opposite directions, f the
 *             lower-numbered one going a -> b, e = (x_b - x_a) / |x_b - x_a|: beta_e = atan2((n_f x n_g) . e, n_f . n_g).
 *             Every other edge (boundary, three or more triangles, traversed twice the same way, zero length, a zero-area
 *             triangle on either side) has beta_e = 0.
 *   mean      H_v = (sum |e| beta_e) / (4 A_v): positive on a convex body with outward normals
 *   tensor6   T_v = (1 / A_v) sum 1/2 |e| beta_e e e^T, stored xx yy zz xy xz yz; trace T_v = 2 H_v
 *   kminmax   [n][4]: H - s, H + s with s = sqrt(max(H^2 - K, 0)); then the eigenvalues m - r, m + r of the tensor in the
 *             tangent plane: n_v the normalised sum of corner angle x n_t, a the coordinate axis of the least |n_v component|
 *             (lowest index on ties), t1 = normalise(a - (a . n_v) n_v), t2 = n_v x t1, S = [ti^T T tj],
 *             m = (s11 + s22) / 2, r = sqrt(((s11 - s22) / 2)^2 + s12^2), theta = 1/2 atan2(2 s12, s11 - s22)
 *   dirs      [n][6]: d_min = w = cos theta t1 + sin theta t2 (the eigenvector of m + r: the tensor collects an edge's
 *             bending along the edge, which is bending across it), then d_max = n_v x w; each with its largest-|component|
 *             entry positive (lowest index on ties)
 *   normals   [n][3] n_v;  boundary [n] 1 where the vertex is an end of an edge with exactly one triangle
 * A vertex with A_v = 0 gets 0 in every field; one whose normal sum is zero or non-finite gets a zero normal, zero tensor
 * eigenvalues and zero directions.  Boundary vertices go through the same formulas: their values are no curvatures.
 * topology [5] = edges | boundary edges | non-manifold edges (three or more triangles) | inconsistent edges (two triangles,
 * same direction) | vertices where H^2 - K < 0 was clipped.  device_ms: the device time between the uploads and the
 * downloads (HIP events).  Every output may be NULL.  One round trip: the uploads, three kernels and two stable radix sorts,
 * the downloads, one wait.  No floating-point atomics: two calls give identical bits.  PF_E_ARG for a vertex id outside
 * 0..n-1, n outside 1..2^31-1, n_faces < 1 or 3 n_faces >= 2^31. */
int pf_curvatures(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces, double* out_area,
                  double* out_gauss, double* out_mean, double* out_tensor6, double* out_kminmax, double* out_dirs,
                  double* out_normals, uint8_t* out_boundary, int64_t* topology, double* device_ms);

/* ---- topology of a triangle mesh: face adjacency, patches, orientability, the faces to reverse, boundary loops ------
 * n vertices, faces [n_faces][3] i32 (host; triangles only), pts [n][3] f64 (host) or NULL: the points only serve the
 * outward rule.  Integers throughout, the signed volume excepted; vertex (bow-tie) manifoldness is not looked at.
 *   half-edge  h = 3 t + j leaves corner j of face t for corner (j + 1) % 3; its edge is the unordered pair of vertices;
 *              the half-edges of an edge are listed in ascending h
 *   edges      one half-edge: boundary edge.  Two: two-face edge, with parity p = 1 when both half-edges run in the same
 *              direction (inconsistent), else 0.  Three or more: non-manifold edge.
 *   face_neighbours [n_faces][3]  the face across the edge of half-edge 3 t + j; -1 on a boundary edge, -2 on a
 *              non-manifold edge
 *   patch [n_faces]  patches are the connected components of the faces joined across two-face edges only, numbered
 *              0 .. P-1 in ascending order of their smallest face (face 0 is in patch 0)
 *   orientable a patch for which rel[t] in {0, 1} exists with rel[a] ^ rel[b] == p on each of its two-face edges; with
 *              rel[root] = 0 for the patch's smallest face rel is unique
 *   flip [n_faces]  0 on a patch that is not orientable (it is left as it is).  On an orientable patch flip = rel if that
 *              reverses at most half of the patch's faces (a tie keeps the root), else rel ^ 1: a mesh with a few reversed
 *              faces gets exactly those back.  Then the outward rule, with PF_TOPOLOGY_OUTWARD in flags and pts given, for
 *              an orientable patch that is closed (none of its faces touches a boundary or non-manifold edge):
 *              V = 1/6 sum over the patch's faces (a, b, c), as flip leaves them, of a . (b x c); V < 0 reverses the
 *              whole patch (flip ^= 1, V = -V).  Only the sign of V decides.  The sum runs over the faces in ascending
 *              order along a fixed tree (256 consecutive terms, 256 of those sums, the rest in order), separate
 *              multiplies and adds, the cross product first, the dot product left to right; no floating-point atomics.
 *   boundary_loop [n_faces][3]  within a patch two boundary edges are linked when they share a vertex; a loop is a
 *              connected component of that relation; loops are numbered 0 .. B-1 in ascending order of their smallest
 *              half-edge.  The loop of each half-edge, -1 for one that is not on a boundary edge.
 *   patch_orientable, patch_volume  [n_faces] as capacity, the first P entries are written: 1 / 0, and V after the rule
 *              (0.0 where the rule does not apply: not closed, not orientable, no pts, no PF_TOPOLOGY_OUTWARD)
 *   report [8] edges | boundary edges | non-manifold edges | inconsistent edges (the first four of pf_curvatures' and
 *              pf_surface_prepare_signed's topology) | P | B (-1 without boundary_loop) | labelling rounds of the patches
 *              | labelling rounds of the loops (0 without boundary edges)
 *   device_ms  between the uploads and the last download (HIP events): it contains the host's reads of the flag
 * Every output may be NULL.  On the device: the half-edges sorted by edge (one stable radix sort), one thread per edge,
 * then a union-find over the faces whose word (parent << 1 | parity) moves by one 64-bit atomicMin: per two-face edge the
 * larger root goes under the smaller, then the paths are compressed, one round after another, each two ordinary launches,
 * until a flag the host reads says that nothing changed.  No kernel waits for another block.  The loops are labelled
 * the same way over the boundary half-edges sorted by (patch, vertex).  Two calls give the same bits in every output.
 * PF_E_ARG for a vertex id outside 0..n-1, n outside 1..2^31-1, n_faces < 1, 3 n_faces >= 2^31 or unknown flags;
 * PF_E_DEGENERATE for a face that repeats a vertex (the message names the first); a zero-area face of three distinct
 * vertices is legal.  PF_E_INTERNAL if the labelling has not settled after n_faces + 1 rounds (it cannot). */
#define PF_TOPOLOGY_OUTWARD 1u
int pf_mesh_topology(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces, uint32_t flags,
                     int32_t* face_neighbours, int32_t* patch, uint8_t* flip, int32_t* boundary_loop, uint8_t* patch_orientable,
                     double* patch_volume, int64_t* report, double* device_ms);

/* ---- uniform resampling of a triangle mesh by clustering (pf_remesh.hip; the reference has none: an extra) ---------
 * pts [n][3] f64, faces [n_faces][3] i32 (triangles; n_faces may be 0: no dual), mass [n] f64 (>= 0, finite), all host.
 * Start from seeds [m] (vertex indices, C[j] = pts[seeds[j]]) or from centroids_in [m][3]; exactly one of the two is given.
 * tests/_remesh_ref.py states the definition in numpy and the device returns its bits.
 *   d2         d2(i, j) = ((dx dx + dy dy) + dz dz), dx = pts[i][0] - C[j][0], ...: separate multiplies and adds, as the
 *              farthest-point sampling and the nearest-neighbour search compute it
 *   assign     label[i] = argmin_j d2(i, j) over all m centroids, the lowest j on ties: exact, whatever the search skips
 *   start      the labels are the assignment to the starting centroids; with n_iter = 0 the call ends here, and with seeds
 *              that are farthest-point samples the labels are that sampling's owner
 *   iteration  update: the members of a cluster in ascending vertex index, cut into consecutive runs of 64; a run is summed
 *              left to right from 0.0 (mass[i] * pts[i][x] for the numerator, mass[i] for the denominator), the run sums
 *              are added left to right from 0.0, C[j] = num / den per coordinate.  A cluster whose den is 0 (no members, or
 *              none with a mass) keeps its centroid.  Then assign.  changed[t] = labels that differ from the iteration
 *              before; the loop stops after the first iteration with changed == 0, or after n_iter
 *   rep, count [m]: the member with the smallest d2 to the cluster's centroid, the lowest vertex on ties, -1 without
 *              members; the number of members
 *   dual       integers only.  A face whose three labels are pairwise distinct is a candidate; it is rotated so that its
 *              smallest label comes first (which keeps its orientation).  The candidates of one set of three labels become
 *              one output triangle, in the orientation most of them have, on a tie in that of the candidate with the lowest
 *              face index.  Output triangles are in lexicographic order of their sorted label triple, which is packed
 *              into one 64-bit key of 3 x 21 bits: m <= 2^21 - 1.  out_faces [n_faces][3], face_src [n_faces] (the lowest
 *              face index among the candidates) and votes [n_faces][2] (candidates for | against the orientation) are
 *              capacities; report[1] rows are written
 *   labels_in  [n] or NULL: the search of the first assignment starts every vertex at the centroid of this label.  It
 *              decides nothing: any labels in 0 .. m - 1 give the same result.  With PF_CLUSTER_UPDATE_ONLY in flags
 *              (labels_in given, n_iter = 1) they are the labels: one update without any assignment, so that `centroids`
 *              is one update step from given labels; labels, rep, count and the dual then describe labels_in
 *   changed    [n_iter] as capacity, report[0] entries are written (none with PF_CLUSTER_UPDATE_ONLY)
 *   report [8] iterations run | output faces | candidate faces | cells of the last assignment's grid | distances evaluated
 *              by all assignments | assignments | 0 | 0
 *   device_ms  between the uploads and the last download (HIP events): it contains the host's reads of changed[t]
 * Every output may be NULL.  One upload, the loop on device buffers with one word read by the host per iteration, one
 * download.  An assignment bins the centroids into a uniform grid of about 2 m cells, starts every vertex at the centroid
 * of its previous label and visits the cells around it ring by ring until a ring's lower bound, taken with slack, is
 * strictly greater than the best distance found.  No floating-point atomics, no kernel waits for another block: two calls
 * give the same bits in every output.  PF_E_ARG for a vertex id, seed or label out of range, n outside 1..2^31-1, m outside
 * 1..n or above 2^21 - 1, 3 n_faces >= 2^31, n_iter < 0, a coordinate or mass that is not finite, a negative mass, both
 * or neither of seeds and centroids_in, unknown flags; PF_E_DEGENERATE for a face that repeats a vertex. */
#define PF_CLUSTER_UPDATE_ONLY 1u
int pf_mesh_cluster(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces, const double* mass,
                    const int64_t* seeds, int64_t m, int32_t n_iter, uint32_t flags, const double* centroids_in,
                    const int32_t* labels_in, int32_t* labels, double* centroids, int32_t* rep, int32_t* count, int32_t* changed,
                    int32_t* out_faces, int32_t* face_src, int32_t* votes, int64_t* report, double* device_ms);

/* ---- distortion and coverage of a correspondence as a map between surfaces (pf_map_quality.hip; an extra) -----------
 * src_pts [n_src][3] f64, src_faces [n_faces][3] i32 (triangles), tgt_pts [n_tgt][3] f64, tgt_normals [n_tgt][3] f64 or
 * NULL, the map as map_vertices [n_src][c] i32 and map_weights [n_src][c] f64, all host.  c = 1: a vertex map, the weights
 * are not read (NULL).  c = 3: the vertices / bary of pf_surface_nd_closest.  A source vertex whose first map vertex is -1
 * is unmapped; the rest of its row is not read.  f64 throughout, separate multiplies and adds, dot products left to
 * right, cross products component by component.  tests/_map_quality_ref.py states the definition in numpy.
 *   image      c = 1: y_i = tgt_pts[T_i].  c = 3: y_i = (w0 x_a + w1 x_b) + w2 x_c per coordinate.  The image normal m_i the
 *              same way from tgt_normals.  The owner of i is T_i; for c = 3 the corner with the largest weight, the lowest
 *              corner on ties.
 *   face       (i0, i1, i2): u = x1 - x0, w = x2 - x0, U = y1 - y0, W = y2 - y0; E = u . u, F = u . w, G = w . w and E', F',
 *              G' likewise from U, W; a_s = |u x w|, a_i = |U x W|.
 *              invalid    a_s is 0 or not finite, or a corner is unmapped: sigma = (0, 0), ratio 0, flags 0, or 8 with an
 *                         unmapped corner
 *              collapsed  valid and a_i == 0: sigma1 = sqrt(((G E' - (2 F) F') + E G') / (a_s a_s)), a numerator below 0
 *                         counting as 0; sigma2 = 0, ratio 0
 *              otherwise  l = sqrt(E), l' = sqrt(E'), p = l' / l, q = ((F' l) / l' - (l' F) / l) / a_s,
 *                         s = (a_i l) / (l' a_s), Q = sqrt(((p + s) / 2)^2 + (q / 2)^2), R = sqrt(((p - s) / 2)^2 + (q / 2)^2),
 *                         sigma1 = Q + R, sigma2 = |Q - R|, ratio = a_i / a_s: the singular values of the linear map
 *                         between the two triangles in their own planes.  The identity gives (1, 1) and 1 exactly, a
 *                         scaling by a power of two that power.
 *              flipped    with tgt_normals only: valid, not collapsed and (U x W) . ((m0 + m1) + m2) < 0
 *   face_sigma [n_faces][2], face_area_ratio [n_faces], face_flags [n_faces] u8: 1 valid | 2 collapsed | 4 flipped |
 *              8 unmapped corner
 *   vertex     over the half-edges h = 3 t + j that leave the vertex, in ascending h, as pf_curvatures sums:
 *              vertex_area A_i = (sum a_s / 2) / 3 over the faces whose a_s is finite and not 0, mapped or not: the area of
 *              pf_curvatures, bit for bit.  vertex_sigma [n_src][2] = (sum (a_s / 2) sigma) / (sum a_s / 2) over the valid
 *              incident faces, 0 without any.  vertex_flags [n_src] u8: the OR of the incident faces' flags.
 *   coverage   target_count [n_tgt] i32: the mapped source vertices the target vertex owns.  target_premass [n_tgt]: the
 *              sum of their A_i, the owned vertices in ascending i cut into consecutive runs of 64, a run summed left to
 *              right from 0.0, the run sums added left to right from 0.0 (the order of pf_mesh_cluster's update).
 *   totals [8] each a sum over the faces in ascending order along the fixed tree of pf_mesh_topology (256 consecutive
 *              terms, 256 of those sums, the rest in order), invalid faces adding 0: source area of the valid faces
 *              sum a_s / 2 | image area sum a_i / 2 | Dirichlet energy 1/2 sum (a_s / 2) (sigma1^2 + sigma2^2) | sum (a_s / 2)
 *              sigma1 | sum (a_s / 2) sigma2 | source area of the collapsed faces | of the flipped faces | 0
 *   report [8] faces: valid | collapsed | flipped (-1 without tgt_normals) | invalid | with an unmapped corner | target
 *              vertices with count > 0 | the largest count | source vertices with a flipped incident face (-1 without
 *              tgt_normals)
 *   device_ms  between the uploads and the downloads (HIP events)
 * Every output may be NULL.  One round trip: the uploads, seven kernels and two stable radix sorts (the half-edges by
 * vertex, the source vertices by owner), the downloads, one wait.  No floating-point atomics (the counts are integer sums
 * and one integer maximum), no kernel waits for another block: two calls give the same bits in every output.  PF_E_ARG
 * for a face index outside 0..n_src-1, a map vertex of a mapped row outside 0..n_tgt-1, c other than 1 or 3, c = 3
 * without weights, n_src or n_tgt outside 1..2^31-1, n_faces < 1 or 3 n_faces >= 2^31, and for a mapped row whose source
 * point, target points, target normals or weights are not finite; PF_E_DEGENERATE for a source face that repeats a
 * vertex.  These checks run on the host before anything is launched. */
int pf_map_distortion(pf_ctx* ctx, const double* src_pts, int64_t n_src, const int32_t* src_faces, int64_t n_faces,
                      const double* tgt_pts, int64_t n_tgt, const double* tgt_normals, const int32_t* map_vertices,
                      const double* map_weights, int32_t c, double* face_sigma, double* face_area_ratio, uint8_t* face_flags,
                      double* vertex_area, double* vertex_sigma, uint8_t* vertex_flags, int32_t* target_count,
                      double* target_premass, double* totals, int64_t* report, double* device_ms);

/* ---- a population of shapes in correspondence: Procrustes alignment and principal modes (pf_shapes.hip; an extra) --------
 * S shapes of n vertices each, vertex i of every shape the same anatomical point: X [S][n][3] f64, optional weights w [n]
 * (vertex areas; NULL: every weight is 1.0) and a reference shape r [n][3] (zeros after create) stay on the device.  The
 * device does elementwise work and sums of a fixed order; every small dense step (3 x 3 SVDs, the S x S eigenproblem) is
 * the caller's.  f64 throughout, separate multiplies and adds; tests/_shape_model_ref.py states the definitions in numpy.
 *   T(.)       the sum over the vertices i in ascending order along the fixed tree of pf_map_distortion's totals: 256
 *              consecutive terms left to right from 0.0, 256 of those sums likewise, the rest in order
 *   dot3(a, b) (a0 b0 + a1 b1) + a2 b2
 *   sums over the shapes go left to right from shape 0
 *   pf_shapes_create         shapes [S][n][3], weights [n] or NULL (host): one upload.  W = T(w_i) is computed once (n
 *                            without weights).  pf_shapes_weight_sum returns W.
 *   pf_shapes_center         c_s[a] = T(w_i x_sia) / W -> centroids_out [S][3] (may be NULL); then x_sia <- x_sia - c_s[a]
 *   pf_shapes_mean           m_i = ((x_first,i + x_first+1,i) + ...) / count per coordinate over the shapes first ..
 *                            first + count - 1 (the sum starts with its first term: count = 1 makes that shape the
 *                            reference bit for bit); change = T(w_i dot3(m_i - r_i, m_i - r_i)) against the reference as
 *                            it was; then m becomes the reference.  mean_out [n][3] and change_out may be NULL.
 *   pf_shapes_align_sums     cross_out [S][9]: H_s[a][b] = T((w_i x_sia) r_ib); norm2_out [S]: q_s = T(w_i dot3(x_si, x_si));
 *                            ref_norm2_out: rho2 = T(w_i dot3(r_i, r_i)).  One pass over the population for all 10 S + 1
 *                            sums.  Each may be NULL.
 *   pf_shapes_transform      R [S][9] (row-major 3 x 3), scale [S], t [S][3] or NULL:
 *                            y_b = scale_s ((x0 R[0][b] + x1 R[1][b]) + x2 R[2][b]), + t_s[b] when t is given; in place
 *   pf_shapes_gram           with d_si = x_si - r_i: gram_out [S][S], G[s][t] = T(w_i dot3(d_si, d_ti)) for s <= t, G[t][s]
 *                            the same bits
 *   pf_shapes_combine        coeff [K][S], 1 <= K <= S -> out [K][n][3], out_k,i,c = sum over s of coeff[k][s] d_si,c, left to
 *                            right from 0.0
 *   pf_shapes_scores         modes [K][n][3], 1 <= K <= 1024 -> scores_out [S][K], b[s][k] = T(w_i dot3(d_si, p_ki))
 *   pf_shapes_set_reference  ref [n][3] becomes r
 *   pf_shapes_download       shapes_out [S][n][3]: the population as it stands
 *   pf_shapes_device_ms      *last_ms (may be NULL) = the device time of the last primitive that ran while the timing was
 *                            on, between its uploads and its downloads (HIP events); then the timing is set to `enable`
 * No floating-point atomics, no kernel waits for another block: two calls give the same bits.  The Gram and the scores run
 * 16 x 16 pairs per block over LDS tiles; their partial sums are kept per 256 vertices while that stays below 1 GiB and per
 * 65 536 vertices beyond (the same terms in the same order either way), so the scratch does not grow like n S^2.
 * PF_E_ARG for S outside 1..1024, n outside 1..2^31-1, K outside 1..S (combine) or 1..1024 (scores), first < 0, count < 1
 * or first + count > S, a coordinate, weight, rotation, scale, translation, coefficient or mode that is not finite, and a
 * negative weight; PF_E_DEGENERATE when W is 0.  These checks run on the host before anything is launched. */
typedef struct pf_shapes pf_shapes;
int pf_shapes_create(pf_ctx* ctx, const double* shapes, int32_t S, int64_t n, const double* weights, pf_shapes** out);
void pf_shapes_free(pf_shapes* h);
int pf_shapes_weight_sum(pf_shapes* h, double* weight_sum);
int pf_shapes_center(pf_shapes* h, double* centroids_out);
int pf_shapes_mean(pf_shapes* h, int32_t first, int32_t count, double* mean_out, double* change_out);
int pf_shapes_align_sums(pf_shapes* h, double* cross_out, double* norm2_out, double* ref_norm2_out);
int pf_shapes_transform(pf_shapes* h, const double* R, const double* scale, const double* t);
int pf_shapes_gram(pf_shapes* h, double* gram_out);
int pf_shapes_combine(pf_shapes* h, const double* coeff, int32_t K, double* out);
int pf_shapes_scores(pf_shapes* h, const double* modes, int32_t K, double* scores_out);
int pf_shapes_set_reference(pf_shapes* h, const double* ref);
int pf_shapes_download(pf_shapes* h, double* shapes_out);
int pf_shapes_device_ms(pf_shapes* h, int32_t enable, double* last_ms);

/* ---- the isosurface of a sampled scalar field: marching tetrahedra (pf_isosurface.hip; the reference has none: an extra) ----
 * values [nx][ny][nz] f64, C-contiguous, host; every extent >= 2; nx ny nz < 2^31.  The sample (i, j, k) sits at
 * origin + (i sx, j sy, k sz) with spacing = (sx, sy, sz).  A lattice point is inside when value < level: a value equal to
 * the level is outside.  tests/_isosurface_ref.py states the definition in numpy and the device returns its bits.
 *   cells      each of the (nx-1)(ny-1)(nz-1) cubes is cut into six tetrahedra, one per permutation (a, b, c) of the axes in
 *              lexicographic order (012 021 102 120 201 210): v0 = p, v1 = v0 + e_a, v2 = v1 + e_b, v3 = p + (1,1,1).  The
 *              cut is the same in every cube, so the face diagonals of neighbouring cubes agree.
 *   vertices   one per lattice edge whose two ends differ in `inside`.  The edges that leave a lattice point p have the
 *              kinds 0..6 = (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1); edges that leave the volume do not
 *              exist.  The key of an edge is 7 ((i ny + j) nz + k) + kind, taken at its lower end p; the vertices are
 *              numbered in ascending key.  Position, always from the lower end p to the upper end q:
 *              t = (level - v_p) / (v_q - v_p), then per coordinate P_c + t (Q_c - P_c) with P_c = origin_c + i_c s_c and
 *              Q_c = origin_c + (i_c + d_c) s_c: separate multiplies and adds.
 *   faces      a tetrahedron with one inside or one outside vertex l gives the triangle (l r0, l r1, l r2) over its other
 *              vertices r0 < r1 < r2 in local order; one with two inside vertices a < b and outside vertices c < d the
 *              quad (ac, ad, bd, bc), split into (ac, ad, bd) and (ac, bd, bc).  Orientation: the normal points from
 *              inside to outside.  A triangle's last two vertices are swapped when, with its vertices at the edge
 *              midpoints of the unit cube, normal . (centroid of the outside corners - centroid of the inside corners) < 0.
 *              Order: ascending cell index (i (ny-1) + j)(nz-1) + k, then the tetrahedra in permutation order, then the
 *              triangles as above.
 *   zero area  triangles of zero area are kept.  They arise where a value equals the level: t is then 0 or 1 and the
 *              vertices of different edges coincide in position.  The connectivity stays that of a manifold.
 *   pf_isosurface_create  the surface stays on the device behind *handle.  report [8] (may be NULL): vertices | faces |
 *              cells with a face | lattice points | cells | 0 | 0 | 0.  device_ms (may be NULL): between the upload and the
 *              last kernel (HIP events); it contains the host's one read of the two totals that size the outputs.  A
 *              surface without vertices is a success with zero counts.  flags must be 0.
 *   pf_isosurface_fetch   pts [V][3] f64, faces [F][3] i32, vertex_key [V] i64 (the edge key of each vertex) or NULL,
 *              face_cell [F] i32 (the cell index of each face) or NULL; pts / faces may be NULL when V / F is 0.
 * Ordinary launches only, no kernel waits for another block; the only atomics are the integer totals: two calls give the
 * same bits.  PF_E_ARG for an extent below 2, 2^31 or more samples, a value, level, spacing or origin that is not finite,
 * flags other than 0, and for a surface of 2^31 or more vertices or with 3 faces >= 2^31 (the message names the count). */
typedef struct pf_isosurface pf_isosurface;
int pf_isosurface_create(pf_ctx* ctx, const double* values, int64_t nx, int64_t ny, int64_t nz, double level, const double* spacing,
                         const double* origin, uint32_t flags, pf_isosurface** handle, int64_t* report, double* device_ms);
int pf_isosurface_fetch(pf_isosurface* h, double* pts, int32_t* faces, int64_t* vertex_key, int32_t* face_cell);
void pf_isosurface_free(pf_isosurface* h);

/* ---- explicit smoothing of a triangle mesh: Laplacian and Taubin fairing (pf_smooth.hip; the reference has none: an extra) ----
 * pts [n][3] f64, faces [n_faces][3] i32 (host; triangles only).  f64 throughout, separate multiplies and adds, sums left to
 * right.  tests/_smoothing_ref.py states the definition in numpy and the device returns its bits.
 *   neighbours N(v): the distinct vertices u != v that share an edge of some face with v, in ascending u.  A face that
 *              repeats a vertex contributes its proper edges only; a half-edge from a vertex to itself is no edge.
 *   kinds      kind [n] u8 = 1 (boundary: v is an end of an edge with exactly one half-edge, as in pf_curvatures) | 2 (pinned:
 *              the caller's pinned[v] != 0) | 4 (movable, below).
 *   weights    PF_SMOOTH_UNIFORM: w_vu = 1.  PF_SMOOTH_COTANGENT: w_vu = max(0, the sum, over the half-edges h = 3 t + j of
 *              the edge {v, u} in ascending h, of the half cotangent at the opposite corner k = (j + 2) % 3 of t).  The half
 *              cotangent at corner k is 0.5 ((a . b) / |a x b|) with a, b the edges that leave the corner for the next corner
 *              and the one after; 0 at all three corners of a triangle where |a x b| is 0 or not finite at one of them.
 *              Computed once from pts, never updated.
 *   sweep      with factor f, every movable vertex: x'_v = x_v + f (s / W - x_v), s the running sum from 0.0 of w_vu x_u over
 *              N(v) in ascending u and W that of the w_vu; with uniform weights s is the plain running sum of the x_u and W
 *              the count as a double.  Every other vertex keeps its bits.  All reads come from the previous sweep (Jacobi).
 *   boundary   PF_SMOOTH_FREE: boundary vertices move like all others.  PF_SMOOTH_FIXED: they do not move.
 *              PF_SMOOTH_CURVE: a boundary vertex sums only the neighbours joined to it by a boundary edge, with weight 1
 *              and W their count, whatever the weights.  A pinned vertex never moves.  movable: not pinned, not a boundary
 *              vertex under PF_SMOOTH_FIXED, and W > 0.
 *   clamp      with bounds c [ncols] >= 0, after every clamp_every-th sweep (the sweeps count from 1), per component of a
 *              movable vertex: x < x0 - c ? x0 - c : x, then x > x0 + c ? x0 + c : x, with x0 the run's input.
 *   stats [6]  (values == NULL only) signed volume of the input, of the result | vertex mean of the result [3] | largest
 *              |x - x0| over all components.  Volume: the sum over the faces in ascending order of x0 . (x1 x x2), the cross
 *              product component-wise, the dot product left to right, along the library's fixed tree (256 consecutive terms
 *              left to right from 0.0, 256 of those sums likewise, the rest in order), divided by 6; the mean: each
 *              coordinate's sum over the vertices along the same tree, divided by n.
 *   pf_smoother_create     uploads once and builds the adjacency (CSR, int32): two stable radix sorts (half-edges by edge key,
 *              directed entries by source vertex), one read-back (the edge count) and a second wait.  pinned [n] may be NULL.
 *   pf_smoother_info       counts [6] = edges | boundary edges | non-manifold edges (three or more half-edges) | entries |
 *              largest row | movable vertices.
 *   pf_smoother_adjacency  rowptr [n + 1], col [entries], w [entries] (1.0 with uniform weights), kind [n]; each may be NULL.
 *   pf_smoother_run        values [n][ncols] (host), or NULL: the mesh's own points (ncols = 3, no upload).  factors
 *              [n_sweeps]: sweep s uses factors[s] (Laplacian: lambda, lambda, ...; Taubin: lambda, mu, lambda, mu, ...).
 *              clamp (may be NULL) [ncols].  out [n][ncols].  One upload, n_sweeps launches that ping-pong two buffers, one
 *              download, one wait; n_sweeps = 0 returns the input's bits.  stats and device_ms (the device time between the
 *              upload and the download, HIP events) may be NULL.
 * No floating-point atomics, no kernel waits for another block: two calls give the same bits.  PF_E_ARG for a vertex id
 * outside 0..n-1, n outside 1..2^31-1, n_faces < 1, 3 n_faces >= 2^31 or 2^31 entries or more, an unknown weights or
 * boundary_mode, ncols outside 1..32 (or not 3 with values == NULL), stats with values, a factor that is not finite, a
 * negative or NaN bound, clamp_every < 1 with a clamp. */
enum { PF_SMOOTH_UNIFORM = 0, PF_SMOOTH_COTANGENT = 1 };
enum { PF_SMOOTH_FREE = 0, PF_SMOOTH_FIXED = 1, PF_SMOOTH_CURVE = 2 };
typedef struct pf_smoother pf_smoother;
int pf_smoother_create(pf_ctx* ctx, const double* pts, int64_t n, const int32_t* faces, int64_t n_faces, int32_t weights,
                       int32_t boundary_mode, const uint8_t* pinned, pf_smoother** handle);
int pf_smoother_info(const pf_smoother* h, int64_t* counts);
int pf_smoother_adjacency(pf_smoother* h, int32_t* rowptr, int32_t* col, double* w, uint8_t* kind);
int pf_smoother_run(pf_smoother* h, const double* values, int32_t ncols, const double* factors, int32_t n_sweeps, int32_t clamp_every,
                    const double* clamp, double* out, double* stats, double* device_ms);
void pf_smoother_free(pf_smoother* h);

/* ---- the exact Euclidean distance transform of a binary volume, with its feature transform (pf_edt.hip; the reference has
 * none: an extra) ----
 * mask [nx][ny][nz] u8, C-contiguous (z fastest), host; every extent >= 1 (a 2-D image is (nx, ny, 1)); nx ny nz < 2^31.  A
 * voxel with mask != 0 is a feature.  spacing = (sx, sy, sz), positive and finite.  tests/_edt_ref.py states the definition
 * in numpy and the device returns its bits.  For a voxel p = (i, j, k) and a feature q = (i', j', k'), the integer
 * differences d_a converted to double, separate multiplies and adds:
 *     t_a(p, q) = (s_a d_a) (s_a d_a)    per axis a
 *     c(p, q)   = (t_z + t_y) + t_x
 *     dist2(p)  = min over all features q of c(p, q);   dist(p) = sqrt(dist2(p))  (the device's double square root)
 *   nearest    is defined in stages, which is what a separable pass computes and keeps every tie decidable:
 *              stage z  the feature k' of p's own z-line with the smallest t_z, the lower k' on a tie: g_z(i, j, k);
 *              stage y  the j' that minimises fl(g_z(i, j', k) + t_y) over the y-line, the lower j' on a tie: g_zy(i, j, k);
 *              stage x  the i' that minimises fl(g_zy(i', j, k) + t_x) over the x-line, the lower i' on a tie.
 *              nearest(p) [N] i32 is the flat index (i' ny + j') nz + k' of the feature that survives.  Addition and
 *              multiplication are monotone, so the staged value is dist2(p) bit for bit and c(p, nearest(p)) == dist2(p)
 *              exactly; where every sum is exact (integer spacings) nearest(p) is the lowest flat index among the minimisers.
 *              A line without a feature carries +inf and -1 through; a volume without one gives dist2 = dist = +inf and
 *              nearest = -1.
 *   signed     PF_EDT_SIGNED: dist(p) = dist_to_foreground(p) - dist_to_background(p), one of which is 0: negative inside
 *              the mask, like pf_surface_signed_distance.  dist2 is the square of the magnitude (the other class's dist2) and nearest
 *              the nearest voxel of the other class.  With an empty class the values are +inf (no foreground) or -inf (no
 *              background) and nearest = -1.
 *   pf_edt_create      one upload; per transform a bit-packing pass, stage z on the packed words (count-leading / -trailing
 *              zeros) and the stages y and x as searches outward from p that stop at t(r) > best; signed mode transforms
 *              the mask and its complement and combines them.  The results stay on the device behind *handle.  report [8]
 *              (may be NULL): samples | foreground | background | 0 ...  device_ms (may be NULL): between the upload and the
 *              last kernel (HIP events).  flags must be 0.
 *   pf_edt_fetch       dist [N] f64, dist2 [N] f64, nearest [N] i32; each may be NULL.
 *   pf_edt_isosurface  the isosurface of the resident dist (the signed field in signed mode) at `level` on the lattice of the
 *              given origin and the handle's spacing: the body of pf_isosurface_create without the download and upload of the
 *              field, with the same outputs and report; the result is a pf_isosurface like any other.
 * Ordinary launches only, no kernel waits for another block, the only atomic is the integer foreground count: two calls
 * give the same bits.  PF_E_ARG for an extent below 1, 2^31 or more samples, a spacing that is not positive and finite, one
 * whose squared distances leave the normal doubles (s s subnormal, or the squared diagonal of the volume not finite: t_a would
 * stop growing with |d_a|), an unknown mode, flags other than 0; pf_edt_isosurface: any extent below 2, a level or origin
 * that is not finite, and a field that is not finite because a class is empty. */
enum { PF_EDT_UNSIGNED = 0, PF_EDT_SIGNED = 1 };
typedef struct pf_edt pf_edt;
int pf_edt_create(pf_ctx* ctx, const uint8_t* mask, int64_t nx, int64_t ny, int64_t nz, const double* spacing, int32_t mode,
                  uint32_t flags, pf_edt** handle, int64_t* report, double* device_ms);
int pf_edt_fetch(pf_edt* h, double* dist, double* dist2, int32_t* nearest);
int pf_edt_isosurface(pf_edt* h, double level, const double* origin, pf_isosurface** out, int64_t* report, double* device_ms);
void pf_edt_free(pf_edt* h);

/* ---- connected components of a mask or a label map, with exact integer statistics (pf_ccl.hip; the reference has none: an
 * extra) ----
 * vol [nx][ny][nz] i32, C-contiguous (z fastest), host; every extent >= 1; N = nx ny nz < 2^31.  tests/_ccl_ref.py states the
 * definition in numpy and the device returns its bytes.
 *   background    a voxel with vol == 0.  connectivity is 6, 18 or 26: neighbours differ by at most 1 on every axis, in at
 *                 most 1, 2 or 3 axes.
 *   modes         PF_CCL_BINARY: two neighbouring voxels are joined if both are non-zero.  PF_CCL_BY_VALUE: if both are
 *                 non-zero and equal.  PF_CCL_BACKGROUND: PF_CCL_BINARY on the complement: the zero voxels are labelled and
 *                 the non-zero ones are the background (what hole filling needs).
 *   components    a component is a class of the transitive closure.  Its root is its lowest flat index (i ny + j) nz + k.
 *                 Components are numbered 1..C by ascending root.  component [N] i32: 0 on the background, otherwise the
 *                 component's number.  In binary mode this is scipy.ndimage.label with generate_binary_structure(3, 1 | 2 | 3),
 *                 numbering included.  Without a labelled voxel C = 0, every label is 0 and the tables are empty.
 *   statistics    per component, exact integers: count i64; value i32, the input at the root (0 in background mode); root i32;
 *                 lo [3], hi [3] i32, the inclusive bounding box in index space; border u8, 1 if a voxel of the component has
 *                 an index of 0 or extent - 1 on any axis; sum [3] i64, the sums of i, j and k.  Centroids in millimetres
 *                 and volumes are host arithmetic on these.
 *   pf_ccl_create one upload; the labelling and the tables stay on the device behind *handle.  Runs along z come from
 *                 bit-packed lines without a union; run starts are joined across the backward half of the neighbouring
 *                 lines by lock-free unions (atomicMin, the larger root under the smaller; a retry means another thread got
 *                 there first and strictly lowers the index retried with, so every launch ends on any input); roots are
 *                 flagged, scanned and numbered; the tables are filled with integer atomics, one per field and wave where a
 *                 wave's voxels share their component.  report [8] (may be NULL): samples | labelled voxels | components |
 *                 retries of the unions | largest count | 0 ...  The retries depend on scheduling: they are the one number
 *                 of a call that two calls need not share.  device_ms (may be NULL): between the upload and the last kernel
 *                 (HIP events; the read-back of C that sizes the tables lies inside).  flags must be 0.
 *   pf_ccl_fetch  component [N] i32, count [C] i64, value [C] i32, root [C] i32, lo [C][3] i32, hi [C][3] i32, border [C] u8,
 *                 sum [C][3] i64; each may be NULL.
 *   pf_ccl_select out [N] u8 = component > 0 && keep[component - 1] (keep [C] u8; may be NULL when C = 0): one gather launch
 *                 and one download.  The host chooses components from the tables, the device applies the choice.
 *   pf_ccl_info   C.
 *   pf_ccl_combine_stats  for measurements: 0 sends every voxel's statistics with atomics of its own (the tables are the
 *                 same bytes either way); 1, the default, combines within a wave.  Process-wide.
 * Ordinary launches only, no kernel waits for another block, no floating point: two calls give the same bytes.  PF_E_ARG for
 * NULL arguments, an extent below 1, 2^31 or more samples, a connectivity other than 6, 18 or 26, an unknown mode, flags
 * other than 0. */
enum { PF_CCL_BINARY = 0, PF_CCL_BY_VALUE = 1, PF_CCL_BACKGROUND = 2 };
typedef struct pf_ccl pf_ccl;
int pf_ccl_create(pf_ctx* ctx, const int32_t* vol, int64_t nx, int64_t ny, int64_t nz, int32_t connectivity, int32_t mode,
                  uint32_t flags, pf_ccl** handle, int64_t* report, double* device_ms);
int pf_ccl_fetch(pf_ccl* h, int32_t* component, int64_t* count, int32_t* value, int32_t* root, int32_t* lo, int32_t* hi,
                 uint8_t* border, int64_t* sum);
int pf_ccl_select(pf_ccl* h, const uint8_t* keep, uint8_t* out);
int pf_ccl_info(const pf_ccl* h, int64_t* n_components);
int pf_ccl_combine_stats(int on);
void pf_ccl_free(pf_ccl* h);

#ifdef __cplusplus
}
#endif
#endif /* PYFOCUSR_HIP_H */

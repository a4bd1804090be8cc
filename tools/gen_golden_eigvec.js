#!/usr/bin/env node
/* Golden vectors of schur_eigenvals, schur_eigen (src/la/schur.js:31-370), eigen_balance_pre and eigen_balance_post
 * (src/la/eigen.js:91-270) from the real reference bundle. The quasi-triangular inputs T are built directly, not through the
 * reference's schur_decomp: the upper triangle from the repo's counter-based generator nd4_uniform (twin of nd4js_amd/rng.py),
 * 2x2 blocks [[a, b], [-c, a]] with b c > 0 at chosen rows, and (mode 'spread') a diagonal of distinct values at least 1.5
 * apart in hashed order, so that eigenvalues are well separated; Q is the reference's qr_decomp of a generated matrix. Only
 * numbers are written: inputs and outputs as .npy (complex as <c16) plus a manifest.json under tests/golden/eigvec/. A case
 * whose reference call throws records the message. For every schur_eigen case with a dense Q the manifest also records the
 * reference's own largest residual ||(Q T Q^T) v - lambda v||_2 / (||T||_F ||v||_2) over the columns (ref_residual; with Q = I:
 * ref_residual_identity_q), the largest | scaled 2-norm - 1 | of its columns (ref_colnorm_err), and the smallest distance
 * of two eigenvalues over ||T||_F.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_eigvec.js
 *
 * Without ND4_REFERENCE the bundle is found through BASELINE.json's reference_path, as the node tests do.
 */
'use strict';
const fs = require('fs'), path = require('path');
const ROOT = path.join(__dirname, '..');
function referenceBundle() {
  if (process.env.ND4_REFERENCE) return process.env.ND4_REFERENCE;
  const base = JSON.parse(fs.readFileSync(path.join(ROOT, 'BASELINE.json')));
  return path.join(base.reference_path, 'dist', 'nd.js');
}
const nd = require(referenceBundle());
const OUT = path.join(ROOT, 'tests', 'golden', 'eigvec');
fs.mkdirSync(OUT, {recursive: true});

/* ---------- the repo's counter-based generator (nd4js_amd/rng.py) ---------- */
function fmix32(h) {
  h ^= h >>> 16; h = Math.imul(h, 0x85ebca6b);
  h ^= h >>> 13; h = Math.imul(h, 0xc2b2ae35);
  h ^= h >>> 16; return h >>> 0;
}
function nd4_uniform(seed, idx) {
  const hi = fmix32((idx ^ fmix32(seed >>> 0)) >>> 0);
  const lo = fmix32((hi + 0x9E3779B9 + idx) >>> 0);
  const m = (hi >>> 5) * 67108864 + (lo >>> 6);
  return m * 2.220446049250313e-16 - 1.0;
}
function fill(seed, n) { const a = new Float64Array(n); for (let i = 0; i < n; i++) a[i] = nd4_uniform(seed, i); return a; }
function hashIdx(seed, i, mod) { return fmix32((fmix32(seed) + Math.imul(i, 0x9E3779B1)) >>> 0) % mod; }

/* ---------- npy + manifest ---------- */
function npy(name, typed, shape, complex) {
  const descr = complex ? '<c16' : typed instanceof Float64Array ? '<f8' : null;
  if (!descr) throw new Error('dtype');
  let hdr = `{'descr': '${descr}', 'fortran_order': False, 'shape': (${shape.join(', ')}${shape.length === 1 ? ',' : ''}), }`;
  const pad = 64 - ((10 + hdr.length + 1) % 64);
  hdr += ' '.repeat(pad % 64) + '\n';
  const head = Buffer.alloc(10);
  head.write('\x93NUMPY', 0, 'latin1'); head[6] = 1; head[7] = 0; head.writeUInt16LE(hdr.length, 8);
  fs.writeFileSync(path.join(OUT, name + '.npy'), Buffer.concat([head, Buffer.from(hdr, 'latin1'), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength)]));
}
const manifest = {rng: 'fmix32-v1', comment: 'no fixture seed has been replaced', cases: {}};
function record(name, meta, tensors) {
  const files = {}, shapes = {};
  for (const [k, a] of Object.entries(tensors)) {
    const complex = a.dtype === 'complex128';
    npy(`${name}.${k}`, complex ? a.data._array : a.data, Array.from(a.shape), complex);
    files[k] = `${name}.${k}.npy`; shapes[k] = Array.from(a.shape);
  }
  manifest.cases[name] = Object.assign({}, meta, {files, shapes});
  console.log('wrote', name);
}
const arr = (shape, data) => new nd.NDArray(Int32Array.from(shape), Float64Array.from(data));
function run(f) { try { return {out: f()}; } catch (e) { return {error: e.message}; } }

/* ---------- quasi-triangular T, orthogonal Q ---------- */
// blocks: first rows of the 2x2 blocks; mode 'uniform': the diagonal as generated, 'spread': distinct values >= 1.5 apart in hashed order
function quasiTri(seed, N, blocks, mode) {
  const t = new Float64Array(N * N);
  for (let i = 0; i < N; i++) for (let j = i; j < N; j++) t[i * N + j] = nd4_uniform(seed, i * N + j);
  if (mode === 'spread') {
    const p = Array.from({length: N}, (_, i) => i);
    for (let i = N - 1; i > 0; i--) { const j = hashIdx(seed + 5, i, i + 1); [p[i], p[j]] = [p[j], p[i]]; }
    for (let i = 0; i < N; i++) t[i * N + i] = 2 * (p[i] - (N >> 1)) + 0.25 * t[i * N + i];
  }
  for (const i of blocks) {
    const j = i + 1, a = t[i * N + i], b = 0.5 + Math.abs(t[i * N + j]), c = 0.25 + Math.abs(nd4_uniform(seed + 9, i));
    t[i * N + i] = a; t[j * N + j] = a; t[i * N + j] = (i & 2) ? -b : b; t[j * N + i] = (i & 2) ? c : -c;
  }
  return t;
}
function orthoQ(seed, N) { return nd.la.qr_decomp(arr([N, N], fill(seed, N * N)))[0]; }
function eye(N) { const a = new Float64Array(N * N); for (let i = 0; i < N; i++) a[i * N + i] = 1; return arr([N, N], a); }
function stack(lead, mats, N) {
  const a = new Float64Array(mats.length * N * N);
  mats.forEach((m, b) => a.set(m.data || m, b * N * N));
  return arr(lead.concat([N, N]), a);
}
function froNorm(t) { let s = 0; for (const x of t) s += x * x; return Math.sqrt(s); }
// the largest residual of one matrix's eigenpairs, and the smallest eigenvalue distance over ||T||_F
function residual(N, q, t, lam, v) {             // q, t real N x N; lam complex [N]; v complex [N, N], all as Float64Arrays
  const nt = froNorm(t);
  let worst = 0, gap = Infinity, norm = 0;
  const x = new Float64Array(2 * N), y = new Float64Array(2 * N), z = new Float64Array(2 * N);
  for (let c = 0; c < N; c++) {
    for (let part = 0; part < 2; part++) {
      for (let k = 0; k < N; k++) { let s = 0; for (let i = 0; i < N; i++) s += q[i * N + k] * v[2 * (i * N + c) + part]; x[2 * k + part] = s; }   // Q^T v
      for (let i = 0; i < N; i++) { let s = 0; for (let k = 0; k < N; k++) s += t[i * N + k] * x[2 * k + part]; y[2 * i + part] = s; }             // T .
      for (let i = 0; i < N; i++) { let s = 0; for (let k = 0; k < N; k++) s += q[i * N + k] * y[2 * k + part]; z[2 * i + part] = s; }             // Q .
    }
    let r2 = 0, v2 = 0;
    const lr = lam[2 * c], li = lam[2 * c + 1];
    for (let i = 0; i < N; i++) {
      const vr = v[2 * (i * N + c)], vi = v[2 * (i * N + c) + 1];
      const rr = z[2 * i] - (lr * vr - li * vi), ri = z[2 * i + 1] - (lr * vi + li * vr);
      r2 += rr * rr + ri * ri; v2 += vr * vr + vi * vi;
    }
    worst = Math.max(worst, Math.sqrt(r2) / (nt * Math.sqrt(v2)));
    let mx = 0, sc = 0;                                                          // | scaled 2-norm of the column - 1 |
    for (let i = 0; i < N; i++) mx = Math.max(mx, Math.abs(v[2 * (i * N + c)]), Math.abs(v[2 * (i * N + c) + 1]));
    for (let i = 0; i < N; i++) { const a = v[2 * (i * N + c)] / mx, b = v[2 * (i * N + c) + 1] / mx; sc += a * a + b * b; }
    norm = Math.max(norm, Math.abs(Math.sqrt(sc) * mx - 1));
    for (let d = 0; d < c; d++) gap = Math.min(gap, Math.hypot(lam[2 * c] - lam[2 * d], lam[2 * c + 1] - lam[2 * d + 1]));
  }
  return {res: worst, gap: N > 1 ? gap / nt : null, norm};
}

/* ---------- schur cases ---------- */
// T [lead..., N, N] (Float64Array), Qd dense Q of the same shape (or null): Lam from schur_eigenvals, VI = schur_eigen(I, T)[1],
// VQ = schur_eigen(Qd, T)[1]
function schurCase(name, meta, lead, N, T, Qd) {
  const batch = lead.reduce((a, b) => a * b, 1), shape = lead.concat([N, N]);
  const Tn = arr(shape, T), tensors = {T: Tn}, m = Object.assign({N, lead}, meta);
  const ev = run(() => nd.la.schur_eigenvals(arr(shape, T)));
  if (ev.error !== undefined) m.eigenvals_error = ev.error; else tensors.Lam = ev.out;
  const I = stack(lead, Array.from({length: batch}, () => eye(N)), N);
  const ri = run(() => nd.la.schur_eigen(I, arr(shape, T)));
  if (ri.error !== undefined) m.eigen_error = ri.error;
  else {
    tensors.VI = ri.out[1];
    const a = ev.out.data._array, b = ri.out[0].data._array;
    for (let i = 0; i < a.length; i++) if (!Object.is(a[i], b[i]) && a[i] !== b[i]) throw new Error(name + ': schur_eigen and schur_eigenvals disagree');
  }
  if (Qd && ri.error === undefined) {
    tensors.Q = Qd;
    const rq = nd.la.schur_eigen(Qd, arr(shape, T));
    tensors.VQ = rq[1];
    let res = 0, gap = Infinity, norm = 0, resI = 0;
    for (let b = 0; b < batch; b++) {
      const sub = (a, n) => a.subarray(b * n, (b + 1) * n);
      const r = residual(N, sub(Qd.data, N * N), sub(T, N * N), sub(rq[0].data._array, 2 * N), sub(rq[1].data._array, 2 * N * N));
      res = Math.max(res, r.res); norm = Math.max(norm, r.norm); if (r.gap !== null) gap = Math.min(gap, r.gap);
      resI = Math.max(resI, residual(N, eye(N).data, sub(T, N * N), sub(ri.out[0].data._array, 2 * N), sub(ri.out[1].data._array, 2 * N * N)).res);
    }
    m.ref_residual = res; m.ref_residual_identity_q = resI; m.ref_colnorm_err = norm; m.min_gap_over_fro = isFinite(gap) ? gap : null;
  }
  record(name, m, tensors);
}
let s = 7000;
const single = (name, N, blocks, mode, dense, extra) => {
  const seed = s; s += 20;
  schurCase(name, Object.assign({seed, blocks, diag: mode}, extra || {}), [], N, quasiTri(seed, N, blocks, mode), dense ? orthoQ(seed + 1, N) : null);
};
// the small tier (T in LDS, N <= 64)
single('n1', 1, [], 'uniform', true);
single('n2_block', 2, [0], 'uniform', true);
single('n3', 3, [1], 'uniform', true);
single('n5', 5, [0, 3], 'uniform', true);
single('n33', 33, [2, 9, 10 + 1, 30], 'spread', true);
single('n33_uniform', 33, [5, 20], 'uniform', true);
single('n64', 64, [0, 17, 40, 62], 'spread', true);
// the blocked tier (N > 64, row blocks of nb = 64 that start at multiples of 64): its smallest N, and 2 nb + 3; the straddle
// variants put a 2x2 block on rows nb-1, nb (and 2nb-1, 2nb), where a block boundary would fall
single('n65', 65, [3, 31, 50], 'spread', true);
single('n65_straddle', 65, [3, 63], 'spread', true, {straddle_rows: [63, 64]});
single('n131', 131, [7, 60, 90, 129], 'spread', true);
single('n131_straddle', 131, [63, 127], 'spread', true, {straddle_rows: [63, 64, 127, 128]});
// batches: members from different seeds
for (const [name, N, blocks, mode] of [['batch_3x2x5', 5, [1], 'uniform'], ['batch_3x2x65', 65, [10, 63], 'spread']]) {
  const seed = s; s += 40;
  const Ts = [], Qs = [];
  for (let b = 0; b < 6; b++) { Ts.push(quasiTri(seed + 3 * b, N, b % 2 ? blocks : blocks.map(i => i + 1), mode)); Qs.push(orthoQ(seed + 3 * b + 1, N)); }
  schurCase(name, {seed, blocks, diag: mode}, [3, 2], N, stack([3, 2], Ts, N).data, stack([3, 2], Qs, N));
}
// restarts and the "set to 0" branch: repeated eigenvalues
schurCase('restart_jordan2', {restart: true}, [], 2, Float64Array.from([1, 1, 0, 1]), orthoQ(s++, 2));
{ const t = quasiTri(s++, 6, [], 'uniform'); t[4 * 6 + 4] = t[1 * 6 + 1];
  schurCase('restart_defective6', {restart: true, rows: [1, 4]}, [], 6, t, orthoQ(s++, 6)); }
schurCase('repeated_nondefective3', {restart: true}, [], 3, Float64Array.from([2, 0, 1, 0, 2, -1, 0, 0, 3]), orthoQ(s++, 3));
{ const t = quasiTri(s++, 131, [40], 'spread'); t[100 * 131 + 100] = t[10 * 131 + 10];
  schurCase('restart_cross_block131', {restart: true, rows: [10, 100]}, [], 131, t, orthoQ(s++, 131)); }
// throw cases
schurCase('throw_real_block', {}, [], 3, Float64Array.from([1, 2, 0.5, 3, 1, -1, 0, 0, 2]), null);
function throwCase(name, f) { const r = run(f); if (r.error === undefined) throw new Error(name + ': the reference did not throw'); manifest.cases[name] = {error: r.error, files: {}, shapes: {}}; console.log('wrote', name); }
throwCase('throw_vals_nonsquare', () => nd.la.schur_eigenvals(arr([2, 3], [1, 2, 3, 4, 5, 6])));
throwCase('throw_eigen_nonsquare', () => nd.la.schur_eigen(arr([2, 3], [1, 2, 3, 4, 5, 6]), arr([2, 3], [1, 2, 3, 4, 5, 6])));
throwCase('throw_eigen_shape', () => nd.la.schur_eigen(eye(2), eye(3)));
throwCase('throw_eigen_ndim', () => nd.la.schur_eigen(eye(2), arr([1, 2, 2], [1, 0, 0, 1])));

/* ---------- balancing ---------- */
function graded(seed, N) { const a = fill(seed, N * N); for (let i = 0; i < N; i++) for (let j = 0; j < N; j++) a[i * N + j] *= Math.pow(2, 3 * (i - j)); return a; }
const pName = p => p === Infinity ? 'inf' : String(p);
function balCase(name, meta, shape, A, p) {
  const r = run(() => nd.la.eigen_balance_pre(arr(shape, A), p));
  const m = Object.assign({p: p === Infinity ? 'Infinity' : p !== p ? 'NaN' : p}, meta);
  if (r.error !== undefined) { m.error = r.error; record(name, m, {A: arr(shape, A)}); return null; }
  record(name, m, {A: arr(shape, A), D: r.out[0], B: r.out[1]});
  return r.out;
}
const balD = {};
for (const N of [1, 2, 7, 64, 200]) balD[N] = balCase(`bal_graded_${N}_p2`, {seed: s}, [N, N], graded(s++, N), 2);
for (const p of [1, 3, Infinity]) for (const N of [7, 64]) balCase(`bal_graded_${N}_p${pName(p)}`, {seed: s}, [N, N], graded(s++, N), p);
{ const a = graded(s++, 7); for (let j = 0; j < 7; j++) a[3 * 7 + j] = 0; balCase('bal_zero_row_7', {}, [7, 7], a, 2); balCase('bal_zero_row_7_pinf', {}, [7, 7], a, Infinity); }
{ const a = fill(s++, 49), b = new Float64Array(49); for (let i = 0; i < 7; i++) for (let j = 0; j < 7; j++) b[i * 7 + j] = a[i * 7 + j] + a[j * 7 + i];
  balCase('bal_balanced_7', {}, [7, 7], b, 2); }
{ const a = new Float64Array(6 * 49); for (let b = 0; b < 6; b++) a.set(graded(s++, 7), b * 49);
  for (const p of [2, Infinity]) balD['b' + pName(p)] = balCase(`bal_batch_2x3x7_p${pName(p)}`, {}, [2, 3, 7, 7], a, p); }
balCase('throw_bal_p_half', {}, [2, 2], [1, 2, 3, 4], 0.5);
balCase('throw_bal_p_nan', {}, [2, 2], [1, 2, 3, 4], NaN);
balCase('throw_bal_nonsquare', {}, [3, 4], fill(s++, 12), 2);
{ const a = graded(s++, 5); a[7] = NaN; balCase('bal_nan_entry_p2', {}, [5, 5], a, 2); balCase('throw_bal_nan_entry_pinf', {}, [5, 5], a, Infinity);
  const b = graded(s++, 5); b[7] = Infinity; balCase('throw_bal_inf_entry_p2', {}, [5, 5], b, 2); }
// eigen_balance_post on the reference's own D (above) and the reference's own eigenvectors of a generated Schur form
function postCase(name, D, lead, N, seed) {
  const batch = lead.reduce((a, b) => a * b, 1), Ts = [], Qs = [];
  for (let b = 0; b < batch; b++) { Ts.push(quasiTri(seed + 3 * b, N, [1 + b % 3], 'spread')); Qs.push(orthoQ(seed + 3 * b + 1, N)); }
  const V = nd.la.schur_eigen(stack(lead, Qs, N), stack(lead, Ts, N))[1];
  record(name, {}, {D, V, W: nd.la.eigen_balance_post(D, V)});
}
postCase('post_7', balD[7][0], [], 7, s); s += 10;
postCase('post_64', balD[64][0], [], 64, s); s += 10;
postCase('post_batch_2x3x7', balD.b2[0], [2, 3], 7, s); s += 30;
throwCase('throw_post_ndim', () => nd.la.eigen_balance_post(arr([3], [1, 2, 3]), arr([3], [1, 2, 3])));
throwCase('throw_post_nonsquare', () => nd.la.eigen_balance_post(arr([2], [1, 2]), arr([2, 3], [1, 2, 3, 4, 5, 6])));

fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest, null, 1) + '\n');

#!/usr/bin/env node
/* Golden vectors of the structure functions from the real reference bundle: NDArray.T, tril / triu (src/la/tri.js:23-42),
 * diag / diag_mat (src/la/diag.js:23-88) and permute_rows / permute_cols / unpermute_rows / unpermute_cols
 * (src/la/permute.js:23-306).
 * Inputs come from the repo's counter-based generator nd4_uniform(seed, idx) (twin of nd4js_amd/rng.py); `special` inputs have
 * NaN, +Infinity, -Infinity, -0 and a denormal planted at hashed positions and, for the tril / triu inputs, NaN and -0 next to
 * the main diagonal on both sides of the cut. Every input and every result is stored: A (and P) and `out`. A refused call stores
 * nothing but its exact message under `errors`, with what is needed to repeat the call (shapes, dtype of P, P's values where
 * they are what is refused). Only numbers and recorded texts are written: .npy files plus manifest.json (with the sha256 of
 * every file) under tests/golden/struct/.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_struct.js
 *
 * Without ND4_REFERENCE the bundle is found through BASELINE.json's reference_path, as the node tests do.
 */
'use strict';
const fs = require('fs'), path = require('path'), crypto = require('crypto');
const ROOT = path.join(__dirname, '..');
function referenceBundle() {
  if (process.env.ND4_REFERENCE) return process.env.ND4_REFERENCE;
  const base = JSON.parse(fs.readFileSync(path.join(ROOT, 'BASELINE.json')));
  return path.join(base.reference_path, 'dist', 'nd.js');
}
const nd = require(referenceBundle());
const OUT = path.join(ROOT, 'tests', 'golden', 'struct');
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
function hashIdx(seed, i, mod) { return fmix32((fmix32(seed >>> 0) + Math.imul(i, 0x9E3779B1)) >>> 0) % mod; }
const prod = s => s.reduce((a, b) => a * b, 1);
const SPECIALS = [NaN, Infinity, -Infinity, -0, 5e-324, -2.5e-310];
function fill(seed, shape, special) {
  const n = prod(shape), a = new Float64Array(n);
  for (let i = 0; i < n; i++) a[i] = nd4_uniform(seed, i);
  if (special && n > 0) {
    SPECIALS.forEach((v, q) => { a[hashIdx(seed, q, n)] = v; });
    // NaN and -0 on both sides of the main diagonal of every matrix (the cut of tril / triu at k = 0 and +-1)
    const M = shape[shape.length - 2], N = shape[shape.length - 1];
    if (shape.length >= 2 && M >= 3 && N >= 3)
      for (let b = 0; b < n / (M * N); b++) {
        const o = b * M * N;
        a[o + N * 1 + 0] = NaN; a[o + N * 0 + 1] = -0; a[o + N * 2 + 1] = -0; a[o + N * 1 + 2] = NaN; a[o + N * 1 + 1] = -0;
      }
  }
  return a;
}
// index vectors: 'perm' a Fisher-Yates permutation, 'identity', 'dup' draws with repetition (some k never named, some twice)
function indexVector(kind, seed, lead, L) {
  const nb = prod(lead), p = new Int32Array(nb * L);
  for (let b = 0; b < nb; b++) {
    const o = b * L;
    if (kind === 'identity') for (let i = 0; i < L; i++) p[o + i] = i;
    else if (kind === 'dup') for (let i = 0; i < L; i++) p[o + i] = hashIdx(seed + b, i, L);
    else {
      for (let i = 0; i < L; i++) p[o + i] = i;
      for (let i = L - 1; i > 0; i--) { const j = hashIdx(seed + b, i, i + 1), t = p[o + i]; p[o + i] = p[o + j]; p[o + j] = t; }
    }
  }
  return p;
}

/* ---------- npy + manifest ---------- */
function npy(file, typed, shape, descr) {
  let hdr = `{'descr': '${descr}', 'fortran_order': False, 'shape': (${shape.join(', ')}${shape.length === 1 ? ',' : ''}), }`;
  const pad = 64 - ((10 + hdr.length + 1) % 64);
  hdr += ' '.repeat(pad % 64) + '\n';
  const head = Buffer.alloc(10);
  head.write('\x93NUMPY', 0, 'latin1'); head[6] = 1; head[7] = 0; head.writeUInt16LE(hdr.length, 8);
  const buf = Buffer.concat([head, Buffer.from(hdr, 'latin1'), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength)]);
  if (buf.length > (1 << 20)) throw new Error(file + ': larger than 1 MiB');
  fs.writeFileSync(path.join(OUT, file), buf);
  return crypto.createHash('sha256').update(buf).digest('hex');
}
const manifest = {rng: 'fmix32-v1', inputs: {}, cases: {}, errors: []};
const arr = (shape, data) => new nd.NDArray(Int32Array.from(shape), data);
function store(table, name, typed, shape) {
  const descr = typed instanceof Int32Array ? '<i4' : '<f8', file = name + '.npy';
  table[name] = {file, shape, dtype: descr === '<i4' ? 'int32' : 'float64', sha256: npy(file, typed, shape, descr)};
}
const INPUT = {};
function input(name, typed, shape) { store(manifest.inputs, name, typed, shape); INPUT[name] = arr(shape, typed); return name; }
function realInput(shape, seed) { const name = 'A_' + (shape.join('x') || 'scalar'); if (!INPUT[name]) input(name, fill(seed, shape, true), shape); return name; }
function golden(name, fn, args, result, extra) {
  const out = {};
  store(out, name + '.out', result.data, Array.from(result.shape));
  manifest.cases[name] = Object.assign({fn, args, out: out[name + '.out']}, extra || {});
  console.log('wrote', name, Array.from(result.shape).join('x'));
}

let seed = 31000;
/* ---------- transposition ---------- */
for (const shape of [[1, 1], [1, 7], [7, 1], [63, 65], [64, 64], [65, 63], [130, 67], [3, 5, 7], [2, 3, 33, 2]]) {
  const a = realInput(shape, seed++);
  golden('T_' + shape.join('x'), 'transpose', {A: a}, INPUT[a].T);
}
/* ---------- tril / triu ---------- */
for (const fn of ['tril', 'triu']) {
  for (const shape of [[5, 8], [8, 5]]) for (const k of [-9, -5, -1, 0, 1, 5, 9]) {
    const a = realInput(shape, seed++);
    golden(`${fn}_${shape.join('x')}_k${k}`, fn, {A: a, k}, nd.la[fn](INPUT[a], k));
  }
  for (const k of [-3, 3]) { const a = realInput([130, 67], seed++); golden(`${fn}_130x67_k${k}`, fn, {A: a, k}, nd.la[fn](INPUT[a], k)); }
  { const a = realInput([3, 5, 7], seed++); golden(`${fn}_3x5x7_default`, fn, {A: a}, nd.la[fn](INPUT[a])); }
}
/* ---------- diag / diag_mat ---------- */
for (const shape of [[5, 8], [8, 5]]) for (let off = -shape[0] + 1; off < shape[1]; off++) {
  const a = realInput(shape, seed++);
  golden(`diag_${shape.join('x')}_o${off}`, 'diag', {A: a, offset: off}, nd.la.diag(INPUT[a], off));
}
for (const off of [-2, 0, 3]) { const a = realInput([3, 5, 7], seed++); golden(`diag_3x5x7_o${off}`, 'diag', {A: a, offset: off}, nd.la.diag(INPUT[a], off)); }
{ const a = realInput([130, 67], seed++); golden('diag_130x67_default', 'diag', {A: a}, nd.la.diag(INPUT[a])); }
for (const shape of [[7], [3, 1], [2, 3, 65]]) {
  const name = input('d_' + shape.join('x'), fill(seed++, shape, true), shape);
  golden('diag_mat_' + shape.join('x'), 'diag_mat', {A: name}, nd.la.diag_mat(INPUT[name]));
}
/* ---------- the four permutation functions ---------- */
const PERM = ['permute_rows', 'permute_cols', 'unpermute_rows', 'unpermute_cols'];
function permCase(fn, tag, aShape, pLead, kind) {
  const cols = fn.endsWith('cols'), L = aShape[aShape.length - (cols ? 1 : 2)];
  const a = realInput(aShape, seed++);
  const pName = `P_${kind}_${pLead.concat([L]).join('x')}`;
  if (!INPUT[pName]) input(pName, indexVector(kind, seed++, pLead, L), pLead.concat([L]));
  const P = INPUT[pName];
  // what the inverse forms leave zero / overwrite, for the tests to assert that the fixture exercises it
  let unnamed = 0, twice = 0;
  for (let b = 0; b < prod(pLead); b++) { const c = new Int32Array(L); for (let i = 0; i < L; i++) c[P.data[b * L + i]]++; for (const x of c) { if (x === 0) unnamed++; if (x > 1) twice++; } }
  golden(`${fn}_${tag}`, fn, {A: a, P: pName}, nd.la[fn](INPUT[a], P), {kind, unnamed, twice});
}
for (const fn of PERM) {
  for (const mn of [[1, 1], [33, 1], [1, 33], [65, 130]]) permCase(fn, `perm_${mn.join('x')}`, mn, [], 'perm');
  permCase(fn, 'identity_65x130', [65, 130], [], 'identity');
  permCase(fn, 'dup_65x130', [65, 130], [], 'dup');
  permCase(fn, 'dup_33x1', [33, 1], [], 'dup');
  permCase(fn, 'dup_1x33', [1, 33], [], 'dup');
  permCase(fn, 'bcastA_9x6', [9, 6], [3], 'perm');                 // A [M,N] with P [3,M]
  permCase(fn, 'bcastP_3x9x6', [3, 9, 6], [1], 'dup');             // A [3,M,N] with P [1,M]
  permCase(fn, 'bcast_2x1x9x6', [2, 1, 9, 6], [3], 'dup');         // A [2,1,M,N] with P [3,M]
  permCase(fn, 'batch_4x5x5', [4, 5, 5], [4], 'perm');
  // one index vector longer than the kernels keep in LDS
  if (fn.endsWith('rows')) { permCase(fn, 'long_4100x3', [4100, 3], [], 'perm'); permCase(fn, 'longdup_4100x3', [4100, 3], [], 'dup'); }
  else { permCase(fn, 'long_2x4100', [2, 4100], [], 'perm'); permCase(fn, 'longdup_2x4100', [2, 4100], [], 'dup'); }
}

/* ---------- refused calls: the exact messages ---------- */
function refused(fn, call, how) {
  let message = null;
  try { call(); } catch (e) { message = e.message; }
  if (message === null) throw new Error(`${fn} ${JSON.stringify(how)}: expected the reference to throw`);
  manifest.errors.push(Object.assign({fn, message}, how));
  console.log('refused', fn, JSON.stringify(how), '->', message);
}
const zeros = shape => arr(shape, new Float64Array(prod(shape)));
const iota = (shape, L) => arr(shape, Int32Array.from({length: prod(shape)}, (_, i) => i % L));
for (const fn of ['tril', 'triu']) for (const shape of [[], [4]]) refused(fn, () => nd.la[fn](zeros(shape)), {a_shape: shape});
for (const shape of [[], [4]]) refused('diag', () => nd.la.diag(zeros(shape)), {a_shape: shape, offset: 0});
for (const [shape, off] of [[[5, 8], -5], [[5, 8], 8], [[8, 5], -8], [[8, 5], 5], [[2, 5, 8], 100]])
  refused('diag', () => nd.la.diag(zeros(shape), off), {a_shape: shape, offset: off});
refused('diag_mat', () => nd.la.diag_mat(zeros([])), {a_shape: []});   // (an empty last axis is refused by NDArray itself)
for (const fn of PERM) {
  const cols = fn.endsWith('cols');
  refused(fn, () => nd.la[fn](zeros([6]), iota([6], 6)), {a_shape: [6], p_shape: [6], p_dtype: 'int32'});
  refused(fn, () => nd.la[fn](zeros([6, 6]), iota([], 1)), {a_shape: [6, 6], p_shape: [], p_dtype: 'int32'});
  refused(fn, () => nd.la[fn](zeros([6, 6]), zeros([6])), {a_shape: [6, 6], p_shape: [6], p_dtype: 'float64'});
  refused(fn, () => nd.la[fn](zeros([4, 6]), iota([cols ? 4 : 6], 4)), {a_shape: [4, 6], p_shape: [cols ? 4 : 6], p_dtype: 'int32'});
  refused(fn, () => nd.la[fn](zeros([2, 6, 6]), iota([3, 6], 6)), {a_shape: [2, 6, 6], p_shape: [3, 6], p_dtype: 'int32'});
  // an index outside [0, L): -1 and L, in a batch whose other members are valid
  for (const bad of [-1, 'L']) {
    const shape = [3, 4, 6], L = cols ? 6 : 4, P = iota([3, L], L);
    P.data[L + 2] = bad === 'L' ? L : -1;
    refused(fn, () => nd.la[fn](zeros(shape), P), {a_shape: shape, p_shape: [3, L], p_dtype: 'int32', p_values: Array.from(P.data), on_device: true});
  }
}

fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest, null, 1) + '\n');

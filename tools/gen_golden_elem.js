#!/usr/bin/env node
/* Golden vectors of elementwise arithmetic and axis reductions from the real reference bundle: nd.zip_elems (src/zip_elems.js),
 * NDArray.mapElems and NDArray.reduceElems (src/nd_array.js:353-360, 464-529) on float64 arrays with the closures of nd.math that
 * are one IEEE operation: add, sub, mul, div, min, max, neg, abs.
 * Inputs come from the repo's counter-based generator nd4_uniform(seed, idx) (twin of nd4js_amd/rng.py), in three kinds:
 *   S  values spread over 2^-40 .. 2^40 with a NaN, +Infinity, -Infinity, +0, -0, a positive and a negative denormal planted at
 *      hashed positions (every zip and map case, min / max reductions, and add / mul reductions with several outputs);
 *   F  finite: a quarter of the values spread as in S, the others within 2^-1 .. 2^1 so that short sums round differently in
 *      different orders; both zeros and the two denormals planted (sums);
 *   P  magnitudes in [0.5, 1.5) with random signs, so that a product of thousands neither overflows nor dies (products).
 * For every add or mul reduction the generator itself folds the same data in reversed order and pairwise and asserts that each of
 * the two differs in at least one non-NaN output's bits from what the reference recorded: a case that cannot tell orders apart
 * would pin nothing (the input of a shape is the first seed that passes in all of its cases). It also asserts that its own fold in the reference's order reproduces the recorded bits.
 * A refused call stores nothing but its exact message under `errors`, with the shapes and arguments that repeat it. Only numbers
 * and recorded texts are written: .npy files plus manifest.json (with the sha256 of every file) under tests/golden/elem/, every
 * file below 100 KB.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_elem.js
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
const OUT = path.join(ROOT, 'tests', 'golden', 'elem');
fs.mkdirSync(OUT, {recursive: true});
for (const f of fs.readdirSync(OUT)) if (f.endsWith('.npy')) fs.unlinkSync(path.join(OUT, f));
const LIMIT = 100 * 1000;

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
// [high word, low word]: +0, -0, the smallest denormal, a negative denormal; then a quiet NaN, +Infinity, -Infinity
const FINITE_WORDS = [[0, 0], [0x80000000, 0], [0, 1], [0x80012345, 0x6789abcd]];
const OTHER_WORDS = [[0x7ff80000, 0], [0x7ff00000, 0], [0xfff00000, 0]];
function fill(kind, seed, n) {
  const a = new Float64Array(n), w = new Uint32Array(a.buffer);
  for (let i = 0; i < n; i++) {
    const u = nd4_uniform(seed, i);
    if (kind === 'P') a[i] = (1 + u / 2) * (hashIdx(seed ^ 0x5bd1e995, i, 2) ? -1 : 1);
    else if (kind === 'F' && hashIdx(seed ^ 0x2545f491, i, 4) !== 0) a[i] = u * Math.pow(2, hashIdx(seed ^ 0x1b873593, i, 3) - 1);
    else a[i] = u * Math.pow(2, hashIdx(seed ^ 0x1b873593, i, 81) - 40);
  }
  if (kind !== 'P' && n >= 12) {
    const words = kind === 'S' ? FINITE_WORDS.concat(OTHER_WORDS) : FINITE_WORDS;
    words.forEach(([hi, lo], q) => { const p = hashIdx(seed, q, n); w[2 * p] = lo; w[2 * p + 1] = hi; });
  }
  return a;
}

/* ---------- npy + manifest ---------- */
function npy(file, typed, shape) {
  let hdr = `{'descr': '<f8', 'fortran_order': False, 'shape': (${shape.join(', ')}${shape.length === 1 ? ',' : ''}), }`;
  const pad = 64 - ((10 + hdr.length + 1) % 64);
  hdr += ' '.repeat(pad % 64) + '\n';
  const head = Buffer.alloc(10);
  head.write('\x93NUMPY', 0, 'latin1'); head[6] = 1; head[7] = 0; head.writeUInt16LE(hdr.length, 8);
  const buf = Buffer.concat([head, Buffer.from(hdr, 'latin1'), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength)]);
  if (buf.length > LIMIT) throw new Error(file + ': larger than ' + LIMIT + ' bytes');
  fs.writeFileSync(path.join(OUT, file), buf);
  return crypto.createHash('sha256').update(buf).digest('hex');
}
const manifest = {rng: 'fmix32-v1', inputs: {}, cases: {}, errors: []};
function entry(name, a) {
  if (a.dtype !== 'float64') throw new Error(name + ': the reference returned dtype ' + a.dtype);
  const shape = Array.from(a.shape), file = name + '.npy';
  return {file, shape, dtype: 'float64', sha256: npy(file, a.data, shape)};
}
const INPUT = {};
let seed = 48000;
// one input per (kind, shape, tag)
function input(kind, shape, tag) {
  const name = `${kind}${tag || ''}_${shape.length ? shape.join('x') : 'scalar'}`;
  if (INPUT[name]) return name;
  INPUT[name] = new nd.NDArray(Int32Array.from(shape), fill(kind, seed++, prod(shape)));
  manifest.inputs[name] = entry(name, INPUT[name]);
  return name;
}
let count = 0;
function golden(name, fn, args, result) {
  if (manifest.cases[name]) throw new Error('duplicate case ' + name);
  manifest.cases[name] = Object.assign({fn}, args, {out: entry(name + '.out', result)});
  count++;
}
const BINARY = ['add', 'sub', 'mul', 'div', 'min', 'max'], UNARY = ['neg', 'abs'], REDUCERS = ['add', 'mul', 'min', 'max'];

/* ---------- zip_elems ---------- */
const ZIPS = [
  ['0d', [], [], BINARY], ['one', [1], [1], BINARY], ['3x5', [3, 5], [3, 5], BINARY], ['4097', [4097], [4097], BINARY],
  ['64x65', [64, 65], [64, 65], BINARY], ['col_row', [70, 1], [1, 130], BINARY], ['row_mat', [130], [70, 130], ['add', 'div', 'min']],
  ['scalar_mat', [], [70, 130], ['sub', 'mul', 'max']], ['mat_scalar', [3, 5], [], BINARY], ['mixed', [2, 1, 3, 1, 2], [5, 1, 4, 1], BINARY],
  ['8axes', [2, 1, 2, 1, 2, 1, 2, 1], [1, 2, 1, 2, 1, 2, 1, 2], BINARY],
  ['10axes', [2, 1, 2, 1, 2, 1, 2, 1, 2, 1], [1, 2, 1, 2, 1, 2, 1, 2, 1, 2], BINARY],
];
for (const [tag, sa, sb, ops] of ZIPS) {
  const a = input('S', sa, 'a'), b = input('S', sb, 'b');
  for (const op of ops) golden(`zip_${op}_${tag}`, 'zip', {op, arrays: [a, b]}, nd.zip_elems([INPUT[a], INPUT[b]], 'float64', nd.math[op]));
}
for (const shape of [[], [3, 5], [4097], [64, 65]]) {
  const a = input('S', shape, 'a');
  for (const op of UNARY) golden(`map_${op}_${shape.length ? shape.join('x') : '0d'}`, 'map', {op, A: a}, INPUT[a].mapElems('float64', nd.math[op]));
}
golden('map_copy_3x5', 'map', {op: null, A: input('S', [3, 5], 'a')}, INPUT[input('S', [3, 5], 'a')].mapElems('float64'));

/* ---------- reduceElems ---------- */
const OPS = {add: (x, y) => x + y, mul: (x, y) => x * y};
const bitsOf = x => { const w = new Uint32Array(Float64Array.of(x).buffer); return w[1] + ':' + w[0]; };      // (both words: a double cannot hold 64 bits)
// the elements of every output in the reference's order: row-major over the reduced axes
function foldLists(shape, red) {
  const nd_ = shape.length, idx = new Array(nd_).fill(0), st = new Array(nd_); let s = 1;
  for (let d = nd_ - 1; d >= 0; d--) { st[d] = s; s *= shape[d]; }
  const ost = new Array(nd_).fill(0); s = 1;
  for (let d = nd_ - 1; d >= 0; d--) if (!red.has(d)) { ost[d] = s; s *= shape[d]; }
  const lists = Array.from({length: s}, () => []);
  for (let e = 0, n = prod(shape); e < n; e++) {
    let o = 0;
    for (let d = 0; d < nd_; d++) o += idx[d] * ost[d];
    lists[o].push(e);
    for (let d = nd_ - 1; d >= 0; d--) { if (++idx[d] < shape[d]) break; idx[d] = 0; }
  }
  return lists;
}
function pairwise(f, xs, lo, hi) {
  if (hi - lo === 1) return xs[lo];
  const mid = (lo + hi) >> 1;
  return f(pairwise(f, xs, lo, mid), pairwise(f, xs, mid, hi));
}
function orderMatters(name, op, A, red, recorded) {
  const f = OPS[op], lists = foldLists(Array.from(A.shape), red);
  let revDiffers = false, pairDiffers = false;
  lists.forEach((list, o) => {
    const xs = list.map(e => A.data[e]);
    const same = xs.slice(1).reduce((acc, x) => f(x, acc), xs[0]);
    const want = recorded.data[o];
    if (!(Number.isNaN(want) ? Number.isNaN(same) : bitsOf(same) === bitsOf(want))) throw new Error(name + ': the generator\'s own ordered fold disagrees with the reference');
    if (Number.isNaN(want) || xs.length < 3) return;
    const rev = xs.slice(0, -1).reduceRight((acc, x) => f(x, acc), xs[xs.length - 1]), pw = pairwise(f, xs, 0, xs.length);
    if (bitsOf(rev) !== bitsOf(want)) revDiffers = true;
    if (bitsOf(pw) !== bitsOf(want)) pairDiffers = true;
  });
  return revDiffers && pairDiffers;
}
const redSet = (axes, nd_) => new Set((typeof axes === 'number' ? [axes] : axes).map(x => x < 0 ? x + nd_ : x));
const folds = (shape, red) => red.size > 0 && prod(shape.filter((_, d) => red.has(d))) >= 3;      // an order exists to be told apart
// The input of the add / mul reductions of one shape: the first seed whose data tells the fold orders apart in every one of them
// (a short fold of a few outputs can round alike in all orders by chance; such data would pin nothing).
function reduceInput(kind, shape, op, axesList) {
  const name = `${kind}r_${shape.join('x')}`;
  if (INPUT[name]) return name;
  for (let tries = 0; tries < 64; tries++) {
    const A = new nd.NDArray(Int32Array.from(shape), fill(kind, seed++, prod(shape)));
    const ok = !OPS[op] || axesList.every(axes => { const red = redSet(axes, shape.length);
      return !folds(shape, red) || orderMatters(name, op, A, red, A.reduceElems(axes, 'float64', nd.math[op])); });
    if (!ok) continue;
    INPUT[name] = A;
    manifest.inputs[name] = entry(name, A);
    return name;
  }
  throw new Error(name + ': no seed tells the fold orders apart');
}
function reduceCase(kind, shape, axes, op, tag, axesList) {
  const a = reduceInput(kind, shape, op, axesList), A = INPUT[a];
  const result = A.reduceElems(axes, 'float64', nd.math[op]);
  const name = `reduce_${op}_${kind}_${shape.join('x')}_${tag}`;
  const red = redSet(axes, shape.length);
  if (OPS[op] && folds(shape, red) && !orderMatters(name, op, A, red, result)) throw new Error(name + ': this data cannot tell the fold orders apart');
  golden(name, 'reduce', {op, A: a, axes}, result);
}
const KIND = {add: 'F', mul: 'P', min: 'S', max: 'S'};
const REDUCTIONS = [
  [[3, 5], 1, 'ax1'], [[3, 5], 0, 'ax0'], [[3, 5], [0, 1], 'all'], [[3, 5], [], 'none'], [[3, 5], [-1, 1, -1], 'dup'],
  [[70, 130], 1, 'ax1'], [[70, 130], 0, 'ax0'], [[130, 70], 1, 'ax1'], [[130, 70], 0, 'ax0'],
  [[1, 4100], 1, 'ax1'], [[4000, 3], 0, 'ax0'], [[5, 67, 9], 1, 'ax1'], [[6, 7, 65], [0, 2], 'ax02'], [[2, 3, 2, 3, 2], [1, 3], 'ax13'],
  [[4099], [0], 'all'],
];
const axesOf = shape => REDUCTIONS.filter(r => r[0].join() === shape.join()).map(r => r[1]);
for (const [shape, axes, tag] of REDUCTIONS) for (const op of REDUCERS) reduceCase(KIND[op], shape, axes, op, tag, axesOf(shape));
// sums and products of data with a NaN, the infinities, zeros and denormals in it: several outputs, so the others still pin the order
for (const op of ['add', 'mul']) { reduceCase('S', [70, 130], 1, op, 'ax1', [1, 0]); reduceCase('S', [70, 130], 0, op, 'ax0', [1, 0]); }
// axes as a 1-D int32 array
{ const a = reduceInput('F', [5, 67, 9], 'add', [1]);
  golden('reduce_add_F_5x67x9_int32axes', 'reduce', {op: 'add', A: a, axes: [2, 0], axes_int32: true},
         INPUT[a].reduceElems(new nd.NDArray(Int32Array.of(2), Int32Array.of(2, 0)), 'float64', nd.math.add)); }

/* ---------- refused calls: the exact messages ---------- */
function refused(fn, how, call) {
  let message = null;
  try { call(); } catch (e) { message = e.message; }
  if (message === null) throw new Error(`${fn} ${JSON.stringify(how)}: expected the reference to throw`);
  manifest.errors.push(Object.assign({fn, message}, how));
}
const zeros = shape => new nd.NDArray(Int32Array.from(shape), new Float64Array(prod(shape)));
for (const shapes of [[[3, 5], [4, 5]], [[3, 5], [3]], [[2, 3], [3, 2]], [[4, 1, 6], [3, 6], [4, 2, 1]], [[2], [3]]])
  refused('zip', {shapes}, () => nd.zip_elems(shapes.map(zeros), 'float64', nd.math.add));
for (const axes of [2, -3, [0, 5], [1, -7], [0, 2]]) refused('reduce', {a_shape: [4, 6], axes}, () => zeros([4, 6]).reduceElems(axes, 'float64', nd.math.add));
refused('reduce', {a_shape: [4, 6], axes_array: {dtype: 'float64', shape: [1], data: [0]}},
        () => zeros([4, 6]).reduceElems(new nd.NDArray(Int32Array.of(1), Float64Array.of(0)), 'float64', nd.math.add));
refused('reduce', {a_shape: [4, 6], axes_array: {dtype: 'int32', shape: [1, 1], data: [0]}},
        () => zeros([4, 6]).reduceElems(new nd.NDArray(Int32Array.of(1, 1), Int32Array.of(0)), 'float64', nd.math.add));
refused('reduce', {a_shape: [4, 6], axes_array: {dtype: 'int32', shape: [], data: [0]}},
        () => zeros([4, 6]).reduceElems(new nd.NDArray(new Int32Array(0), Int32Array.of(0)), 'float64', nd.math.add));

fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest, null, 1) + '\n');
console.log(`wrote ${count} cases, ${Object.keys(manifest.inputs).length} inputs, ${manifest.errors.length} refusals`);
for (const e of manifest.errors) console.log('refused', e.fn, JSON.stringify(e.shapes || e.axes || e.axes_array), '->', e.message);

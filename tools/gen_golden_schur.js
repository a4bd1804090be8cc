#!/usr/bin/env node
/* Golden vectors of schur_decomp (src/la/schur.js:372-683), eigen and eigenvals (src/la/eigen.js:33-88) from the real reference
 * bundle. Per case: the reference's hessenberg_decomp(A) = (U, H) and schur_decomp(A) = (Q, T), its own residual
 * ||Q T Q^T - A||_F / ||A||_F (ref_residual), ||Q^T Q - I||_F (ref_orth) and the seconds the call took (ref_seconds); for single
 * finite matrices also eigen(A): Lam, the largest column residual ||A v - lambda v||_2 / (||A||_F ||v||_2) (ref_eig_residual)
 * and the largest | scaled 2-norm of a column - 1 | (ref_eig_colnorm_err); eigenvals(A) is checked to have eigen's bits.
 * Inputs: 'uniform' cases are the repo's counter-based generator nd4_uniform(seed, idx) (twin of nd4js_amd/rng.py) and are not
 * stored; 'hessenberg' cases are its upper-Hessenberg part with exact zeros planted at subdiagonal rows `zeros` (entry
 * [i, i-1]), for which the reference's hessenberg_decomp returns U = I and H = A bit for bit (asserted here), so U, H and A are
 * not stored either; every other input is stored as A. Only numbers are written: .npy files plus manifest.json (with the sha256
 * of every file) under tests/golden/schur/.
 *
 *   ND4_REFERENCE=<path to dist/nd.js> node tools/gen_golden_schur.js
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
const OUT = path.join(ROOT, 'tests', 'golden', 'schur');
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

/* ---------- npy + manifest ---------- */
function npy(name, typed, shape, complex) {
  let hdr = `{'descr': '${complex ? '<c16' : '<f8'}', 'fortran_order': False, 'shape': (${shape.join(', ')}${shape.length === 1 ? ',' : ''}), }`;
  const pad = 64 - ((10 + hdr.length + 1) % 64);
  hdr += ' '.repeat(pad % 64) + '\n';
  const head = Buffer.alloc(10);
  head.write('\x93NUMPY', 0, 'latin1'); head[6] = 1; head[7] = 0; head.writeUInt16LE(hdr.length, 8);
  const buf = Buffer.concat([head, Buffer.from(hdr, 'latin1'), Buffer.from(typed.buffer, typed.byteOffset, typed.byteLength)]);
  if (buf.length > (1 << 20)) throw new Error(name + ': larger than 1 MiB');
  fs.writeFileSync(path.join(OUT, name + '.npy'), buf);
  return crypto.createHash('sha256').update(buf).digest('hex');
}
const manifest = {rng: 'fmix32-v1', comment: 'no fixture seed has been replaced', cases: {}};
const arr = (shape, data) => new nd.NDArray(Int32Array.from(shape), Float64Array.from(data));

/* ---------- measures ---------- */
function fro(a) { let s = 0; for (const x of a) s += x * x; return Math.sqrt(s); }
function schurErrors(N, a, q, t) {            // [||Q T Q^T - A||_F / ||A||_F, ||Q^T Q - I||_F] of one matrix
  const qt = new Float64Array(N * N);
  for (let i = 0; i < N; i++) for (let k = 0; k < N; k++) { const x = q[N * i + k]; for (let j = 0; j < N; j++) qt[N * i + j] += x * t[N * k + j]; }
  let err = 0, orth = 0;
  for (let i = 0; i < N; i++) for (let j = 0; j < N; j++) {
    let s = 0, o = 0;
    for (let k = 0; k < N; k++) { s += qt[N * i + k] * q[N * j + k]; o += q[N * k + i] * q[N * k + j]; }
    err += (s - a[N * i + j]) ** 2; orth += (o - (i === j ? 1 : 0)) ** 2;
  }
  const na = fro(a);
  return [na > 0 ? Math.sqrt(err) / na : Math.sqrt(err), Math.sqrt(orth)];
}
function eigErrors(N, a, lam, v) {            // lam complex [N], v complex [N, N] as interleaved Float64Arrays
  const na = fro(a);
  let worst = 0, norm = 0;
  for (let c = 0; c < N; c++) {
    let r2 = 0, v2 = 0, mx = 0, sc = 0;
    const lr = lam[2 * c], li = lam[2 * c + 1];
    for (let i = 0; i < N; i++) {
      let sr = 0, si = 0;
      for (let k = 0; k < N; k++) { sr += a[N * i + k] * v[2 * (k * N + c)]; si += a[N * i + k] * v[2 * (k * N + c) + 1]; }
      const vr = v[2 * (i * N + c)], vi = v[2 * (i * N + c) + 1];
      const rr = sr - (lr * vr - li * vi), ri = si - (lr * vi + li * vr);
      r2 += rr * rr + ri * ri; v2 += vr * vr + vi * vi;
      mx = Math.max(mx, Math.abs(vr), Math.abs(vi));
    }
    for (let i = 0; i < N; i++) { const x = v[2 * (i * N + c)] / mx, y = v[2 * (i * N + c) + 1] / mx; sc += x * x + y * y; }
    worst = Math.max(worst, Math.sqrt(r2) / ((na > 0 ? na : 1) * Math.sqrt(v2)));
    norm = Math.max(norm, Math.abs(Math.sqrt(sc) * mx - 1));
  }
  return [worst, norm];
}
const same = (x, y) => x === y || (x !== x && y !== y);

/* ---------- one case ---------- */
// input: {kind: 'uniform', seed} | {kind: 'hessenberg', seed, zeros} | {kind: 'file'}; A is the flat Float64Array [lead..., N, N]
function schurCase(name, family, lead, N, A, input, opts) {
  opts = opts || {};
  const shape = lead.concat([N, N]), batch = lead.reduce((x, y) => x * y, 1);
  const [U, H] = nd.la.hessenberg_decomp(arr(shape, A));
  const t0 = process.hrtime.bigint();
  const [Q, T] = nd.la.schur_decomp(arr(shape, A));
  const secs = Number(process.hrtime.bigint() - t0) / 1e9;
  const m = {family, N, lead, input, ref_seconds: secs, files: {}, shapes: {}, sha256: {}};
  const put = (k, a, complex) => {
    const sh = Array.from(a.shape);
    m.sha256[k] = npy(`${name}.${k}`, complex ? a.data._array : a.data, sh, complex);
    m.files[k] = `${name}.${k}.npy`; m.shapes[k] = sh;
  };
  if (input.kind === 'hessenberg') {
    for (let b = 0; b < batch; b++) for (let i = 0; i < N; i++) for (let j = 0; j < N; j++) {
      const x = b * N * N + N * i + j;
      if (U.data[x] !== (i === j ? 1 : 0) || !same(H.data[x], A[x])) throw new Error(name + ': hessenberg_decomp of a Hessenberg input is not (I, A)');
    }
  } else { put('U', U); put('H', H); }
  if (input.kind === 'file') put('A', arr(shape, A));
  put('Q', Q); put('T', T);
  let finite = true;
  for (const x of A) if (!isFinite(x)) finite = false;
  if (finite) {
    let res = 0, orth = 0;
    for (let b = 0; b < batch; b++) {
      const sub = a => a.subarray(b * N * N, (b + 1) * N * N);
      const [r, o] = schurErrors(N, sub(A), sub(Q.data), sub(T.data));
      res = Math.max(res, r); orth = Math.max(orth, o);
    }
    m.ref_residual = res; m.ref_orth = orth;
  }
  if (finite && batch === 1 && !opts.no_eigen) {
    const [L, V] = nd.la.eigen(arr(shape, A)), L2 = nd.la.eigenvals(arr(shape, A));
    const l = L.data._array, l2 = L2.data._array;
    for (let i = 0; i < l.length; i++) if (!same(l[i], l2[i])) throw new Error(name + ': eigen and eigenvals disagree');
    put('Lam', L, true);
    const [r, c] = eigErrors(N, A, l, V.data._array);
    m.ref_eig_residual = r; m.ref_eig_colnorm_err = c;
  }
  manifest.cases[name] = m;
  console.log('wrote', name, secs.toFixed(4) + ' s');
}

function hessenberg(seed, N, zeros) {
  const a = fill(seed, N * N);
  for (let i = 0; i < N; i++) for (let j = 0; j + 1 < i; j++) a[N * i + j] = 0;
  for (const i of zeros) a[N * i + i - 1] = 0;
  return a;
}
function cyclic(N, down) { const a = new Float64Array(N * N); for (let i = 0; i < N; i++) { if (down) a[N * ((i + 1) % N) + i] = 1; else a[N * i + (i + 1) % N] = 1; } return a; }
function symmetric(seed, N) { const g = fill(seed, N * N), a = new Float64Array(N * N); for (let i = 0; i < N; i++) for (let j = 0; j <= i; j++) a[N * i + j] = a[N * j + i] = g[N * i + j]; return a; }
function rotBlocks(N) {                        // 2x2 rotations by distinct angles on the diagonal: complex pairs on the unit circle
  const a = new Float64Array(N * N);
  for (let i = 0; i + 1 < N; i += 2) { const th = 0.3 + 0.04 * i, c = Math.cos(th), s = Math.sin(th); a[N * i + i] = c; a[N * i + i + 1] = -s; a[N * (i + 1) + i] = s; a[N * (i + 1) + i + 1] = c; }
  return a;
}

let s = 9000;
for (const N of [1, 2, 3, 4, 5, 8, 16, 33, 47, 63, 64, 65, 96, 128, 160]) { const seed = s++; schurCase(`dense_${N}`, 'dense', [], N, fill(seed, N * N), {kind: 'uniform', seed}); }
for (const N of [3, 4, 8, 64, 100]) schurCase(`cyclic_${N}`, 'cyclic', [], N, cyclic(N, N === 4 || N === 100), {kind: 'file'});
for (const N of [2, 8, 64]) schurCase(`sym_${N}`, 'symmetric', [], N, symmetric(s++, N), {kind: 'file'});
schurCase('two_hij_zero', 'special', [], 2, Float64Array.from([1, 0, 2, 3]), {kind: 'file'});
schurCase('two_rotation', 'special', [], 2, Float64Array.from([0.6, -0.8, 0.8, 0.6]), {kind: 'file'});
schurCase('zero_8', 'special', [], 8, new Float64Array(64), {kind: 'file'});
{ const a = new Float64Array(64); for (let i = 0; i < 8; i++) a[9 * i] = 1; schurCase('identity_8', 'special', [], 8, a, {kind: 'file'}); }
{ const a = new Float64Array(64); for (let i = 0; i < 7; i++) a[8 * i + i + 1] = 1; schurCase('jordan_upper_8', 'special', [], 8, a, {kind: 'file'}); }
{ const a = new Float64Array(64); for (let i = 0; i < 7; i++) a[8 * (i + 1) + i] = 1; schurCase('jordan_lower_8', 'special', [], 8, a, {kind: 'file'}); }
for (const N of [8, 64]) schurCase(`rotblocks_${N}`, 'special', [], N, rotBlocks(N), {kind: 'file'});
for (const [N, zeros] of [[16, [8]], [48, [28, 40]], [64, [20, 41]], [160, [50, 100, 130, 145]]]) {
  const seed = s++;
  schurCase(`hess_${N}`, 'hessenberg', [], N, hessenberg(seed, N, zeros), {kind: 'hessenberg', seed, zeros});
}
{ const seed = s++; schurCase('batch_3x2x16', 'dense', [3, 2], 16, fill(seed, 6 * 256), {kind: 'uniform', seed}); }
{ const seed = s++; const a = fill(seed, 3 * 64); a[64 + 8 * 2 + 5] = NaN; schurCase('batch_nan_3x8', 'nan', [3], 8, a, {kind: 'file', nan_member: 1}); }

fs.writeFileSync(path.join(OUT, 'manifest.json'), JSON.stringify(manifest, null, 1) + '\n');

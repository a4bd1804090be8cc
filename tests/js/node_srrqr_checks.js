'use strict';
/* Node-side checks of the strong rank-revealing QR and URV (srrqr_decomp_full, urv_decomp_full, urv_lstsq) through the JS host and the N-API addon.
 * Driven by tests/test_node_srrqr.py.
 *   node node_srrqr_checks.js cpu                        (no GPU: argument checks, loud failure)
 *   node node_srrqr_checks.js install <reference dist/nd.js>   (routing of the three names, minWork forwarding)
 *   node node_srrqr_checks.js gpu <golden dir>           (GPU: results against the reference's goldens; never reads the reference)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['srrqr_decomp_full', 'urv_decomp_full', 'urv_lstsq'];

function fmix32(h) { h ^= h >>> 16; h = Math.imul(h, 0x85ebca6b); h ^= h >>> 13; h = Math.imul(h, 0xc2b2ae35); h ^= h >>> 16; return h >>> 0; }
function uniform(seed, idx) {
  const hi = fmix32((idx ^ fmix32(seed >>> 0)) >>> 0), lo = fmix32((hi + 0x9E3779B9 + idx) >>> 0);
  return ((hi >>> 5) * 67108864 + (lo >>> 6)) * 2.220446049250313e-16 - 1.0;
}
function hashIdx(seed, i, mod) { return fmix32((fmix32(seed) + Math.imul(i, 0x9E3779B1)) >>> 0) % mod; }
function data(seed, n) { const d = new Float64Array(n); for (let i = 0; i < n; i++) d[i] = uniform(seed, i); return d; }
function input(NDA, seed, shape, fam) {          // tools/gen_golden_srrqr.js input() for the families used below
  const M = shape[shape.length - 2], N = shape[shape.length - 1], a = data(seed, shape.reduce((p, q) => p * q, 1));
  if (fam === 'rankdef') {
    const rank = Math.max(1, Math.min(M, N) >> 1);
    for (let i = rank; i < M; i++) for (let j = 0; j < N; j++) a[i * N + j] = 0.5 * a[((i - rank) % rank) * N + j] - 0.25 * a[((i + 1) % rank) * N + j];
  } else if (fam !== 'dense') throw new Error(fam);
  return new NDA(Int32Array.from(shape), a);
}
function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const descr = /'descr': '([^']+)'/.exec(hdr)[1];
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  return descr === '<f8' ? new Float64Array(ab) : new Int32Array(ab);
}
function relerr(x, ref) { let n = 0, d = 0; for (let i = 0; i < ref.length; i++) { d += (x[i] - ref[i]) ** 2; n += ref[i] ** 2; } return Math.sqrt(d / Math.max(n, 1e-300)); }
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;


if (mode === 'cpu') {
  const I = new la.NDArray(Int32Array.of(3, 3), Float64Array.of(1, 0, 0, 0, 1, 0, 0, 0, 1));
  for (const n of NAMES) assert.strictEqual(typeof la[n], 'function', n);
  assert.throws(() => la.srrqr_decomp_full([1, 2, 3]), /^Error: srrqr_decomp_full\(A,opt\): A must be at least 2D\.$/);
  assert.throws(() => la.srrqr_decomp_full(I, {dtol: 0.5}), /^Error: srrqr_decomp_full\(A,opt\): Invalid opt\.dtol: 0\.5\. Must be >=1\.$/);
  assert.throws(() => la.srrqr_decomp_full(I, {ztol: -1}), /^Error: srrqr_decomp_full\(A,opt\): invalid opt\.ztol: -1\. Must be non-negative number\.$/);
  assert.throws(() => la.srrqr_decomp_full(I, {dtol: I}), /NDArray as opt\.dtol not yet supported\./);
  assert.throws(() => la.srrqr_decomp_full(I, {dtol: Infinity}), /^Error: Assertion failed\. Invalid dtol: Infinity\.$/);
  assert.throws(() => la.urv_lstsq(I, I, I), /Either 2 \(\[U,R,V,ranks\], Y\) or 5 arguments/);
  assert.throws(() => la.urv_lstsq(I, I, [1, 2, 3], 3, I), /urv_lstsq\(U,R,V, Y\): V\.ndim must be at least 2\./);
  assert.throws(() => la.urv_lstsq(I, [[1, 0], [0, 1]], I, 3, I), /Matrix dimensions incompatible\./);
  if (la.device_count() === 0)
    for (const f of [() => la.srrqr_decomp_full(I), () => la.urv_decomp_full(I)]) assert.throws(f, /no HIP device/);
  console.log('node srrqr cpu checks ok');
}

if (mode === 'install') {
  const nd = require(process.argv[3]);
  const host = {}; for (const n of NAMES) host[n] = nd.la[n];
  const nd2 = la.install(nd, {minWork: 1e5});
  const orig = nd2.la.__nd4hip_original__;
  for (const n of NAMES) {
    assert.strictEqual(typeof nd2.la[n], 'function', n);
    assert.notStrictEqual(nd2.la[n], host[n], n + ' is not routed');
    assert.strictEqual(orig[n], host[n], n);
  }
  // tiny float64 calls go to the host module's own functions: bit-identical to them
  const A = input(nd.NDArray, 5, [6, 6], 'rankdef'), y = input(nd.NDArray, 7, [6, 2], 'dense');
  const got = nd2.la.srrqr_decomp_full(A), want = host.srrqr_decomp_full(A);
  got.forEach((g, k) => assert.ok(sameBits(g.data, want[k].data), 'srrqr ' + k));
  const u = host.urv_decomp_full(A), gu = nd2.la.urv_decomp_full(A);
  gu.forEach((g, k) => assert.ok(sameBits(g.data, u[k].data), 'urv ' + k));
  assert.ok(sameBits(nd2.la.urv_lstsq(u, y).data, host.urv_lstsq(u, y).data));
  assert.ok(sameBits(nd2.la.urv_lstsq(...u, y).data, host.urv_lstsq(...u, y).data));
  if (la.device_count() === 0) {                    // 128^3 >= minWork: the accelerated path, which fails loudly here
    const B = input(nd.NDArray, 9, [128, 128], 'dense');
    for (const f of [() => nd2.la.srrqr_decomp_full(B), () => nd2.la.urv_decomp_full(B)]) assert.throws(f, /no HIP device/);
  }
  console.log('node srrqr install checks ok');
}

if (mode === 'gpu') {
  const dir = path.join(process.argv[3], 'srrqr');
  const man = JSON.parse(fs.readFileSync(path.join(dir, 'manifest.json'))).cases;
  const ld = (m, k) => loadNpy(path.join(dir, m.files[k]));
  for (const name of ['dense_48x48', 'rankdef_60x40', 'dense_40x60', 'batch5x24']) {
    const m = man[name], A = input(la.NDArray, m.seed, m.shape, m.family);
    const [Q, R, P, r] = la.srrqr_decomp_full(A);
    assert.ok(sameBits(P.data, ld(m, 'P')), name + ' P');
    assert.ok(sameBits(r.data, ld(m, 'r')), name + ' r');
  }
  for (const name of ['urvls_rankdef_48', 'urvls_rankdef_60x40', 'urvls_rankdef_40x60']) {
    const m = man[name], A = input(la.NDArray, m.seed, m.shape, m.family);
    const N = m.shape[0], y = new la.NDArray(Int32Array.of(N, m.J), data(m.y_seed, N * m.J));
    const x = la.urv_lstsq(la.urv_decomp_full(A), y);
    assert.ok(relerr(x.data, ld(m, 'x')) < 1e-10, name);
  }
  console.log('node srrqr gpu checks ok');
}

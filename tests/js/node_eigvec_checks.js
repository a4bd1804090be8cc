'use strict';
/* Node-side checks of schur_eigenvals, schur_eigen, eigen_balance_pre and eigen_balance_post through the JS host and the N-API
 * addon. Driven by tests/test_node_eigvec.py.
 *   node node_eigvec_checks.js cpu                               (no GPU: argument checks)
 *   node node_eigvec_checks.js install <reference dist/nd.js>    (routing of the names)
 *   node node_eigvec_checks.js gpu <golden dir>                  (GPU: one fixture per function against the reference's goldens;
 *                                                                 never reads the reference: a stand-in with its own
 *                                                                 Complex128Array stands in for nd4js)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['schur_eigenvals', 'schur_eigen', 'eigen_balance_pre', 'eigen_balance_post'];

function loadNpy(file) {
  const buf = fs.readFileSync(file), hlen = buf.readUInt16LE(8), hdr = buf.toString('latin1', 10, 10 + hlen);
  const descr = /'descr': '([^']+)'/.exec(hdr)[1], shape = /'shape': \(([^)]*)\)/.exec(hdr)[1].split(',').filter(x => x.trim()).map(Number);
  const body = buf.slice(10 + hlen), ab = body.buffer.slice(body.byteOffset, body.byteOffset + body.byteLength);
  return {data: new Float64Array(ab), shape, complex: descr === '<c16'};
}
const sameValues = (a, b, what) => { assert.strictEqual(a.length, b.length, what); for (let i = 0; i < a.length; i++) assert(a[i] === b[i], `${what}: entry ${i} is ${a[i]}, the reference has ${b[i]}`); };

if (mode === 'cpu') {
  for (const n of NAMES) assert.strictEqual(typeof la[n], 'function', n);
  const W = new la.NDArray(Int32Array.of(2, 3), new Float64Array(6)), S2 = new la.NDArray(Int32Array.of(2, 2), new Float64Array(4)),
        S3 = new la.NDArray(Int32Array.of(3, 3), new Float64Array(9)), B2 = new la.NDArray(Int32Array.of(1, 2, 2), new Float64Array(4));
  assert.throws(() => la.schur_eigenvals(W), /^Error: T is not square\.$/);
  assert.throws(() => la.schur_eigen(W, W), /^Error: Q is not square\.$/);
  assert.throws(() => la.schur_eigen(S2, S3), /^Error: Q\.shape != T\.shape\.$/);
  assert.throws(() => la.schur_eigen(S2, B2), /^Error: Q\.ndim != T\.ndim\.$/);
  assert.throws(() => la.eigen_balance_pre(S2, 0.5), /^Error: Invalid norm p=0\.5;$/);
  assert.throws(() => la.eigen_balance_pre(S2, NaN), /^Error: Invalid norm p=NaN;$/);
  assert.throws(() => la.eigen_balance_pre(W), /^Error: A is not square$/);
  assert.throws(() => la.eigen_balance_post([1, 2], [1, 2]), /^Error: eigen_balance_post\(D,V\): V\.ndim must be at least 2\.$/);
  assert.throws(() => la.eigen_balance_post([1, 2], W), /^Error: eigen_balance_post\(D,V\): V must be square\.$/);
  console.log('node eigvec cpu checks ok');
} else if (mode === 'install') {
  const nd = require(process.argv[3]);
  const before = {};
  for (const n of NAMES) before[n] = nd.la[n];
  const L = la.install(nd, {}).la;
  for (const n of NAMES) { assert.strictEqual(typeof L[n], 'function', n); assert.strictEqual(L.__nd4hip_original__[n], before[n], n); assert.notStrictEqual(L[n], before[n], n); }
  const F = nd.array('float32', [[1, 2], [3, 4]]);                                  // float32 is forwarded to the host module
  assert.strictEqual(L.eigen_balance_pre(F)[1].dtype, 'float32');
  console.log('node eigvec install checks ok');
} else if (mode === 'gpu') {
  class Complex128Array {
    constructor(buffer, byteOffset, length) {
      this._array = new Float64Array(buffer, byteOffset, 2 * length);
      return new Proxy(this, {get: (t, k) => typeof k !== 'symbol' && k % 1 === 0 ? [t._array[2 * k], t._array[2 * k + 1]] : t[k]});
    }
    get length() { return this._array.length / 2; }
  }
  class HostNDArray {
    constructor(shape, data) { this.shape = shape; this.data = data; }
    get ndim() { return this.shape.length; }
    get dtype() { return this.data instanceof Complex128Array ? 'complex128' : this.data instanceof Float64Array ? 'float64' :
                         this.data instanceof Int32Array ? 'int32' : this.data instanceof Float32Array ? 'float32' : 'object'; }
  }
  const L = la.install({NDArray: HostNDArray, dt: {Complex128Array}, la: {matmul2: () => 'host'}}).la;
  const G = path.join(process.argv[3], 'eigvec');
  const cases = JSON.parse(fs.readFileSync(path.join(G, 'manifest.json'))).cases;
  const arr = (name, key) => {
    const x = loadNpy(path.join(G, cases[name].files[key])), n = x.shape.reduce((a, b) => a * b, 1);
    return new HostNDArray(Int32Array.from(x.shape), x.complex ? new Complex128Array(x.data.buffer, 0, n) : x.data);
  };
  const N = 33, eye = new Float64Array(N * N); for (let i = 0; i < N; i++) eye[i * N + i] = 1;
  const lam = L.schur_eigenvals(arr('n33', 'T'));
  assert(lam instanceof HostNDArray && lam.data instanceof Complex128Array);
  assert.deepStrictEqual(Array.from(lam.shape), [N]);
  sameValues(lam.data._array, arr('n33', 'Lam').data._array, 'schur_eigenvals n33');
  const [l2, V] = L.schur_eigen(new HostNDArray(Int32Array.of(N, N), eye), arr('n33', 'T'));
  sameValues(l2.data._array, arr('n33', 'Lam').data._array, 'schur_eigen n33 Lam');
  sameValues(V.data._array, arr('n33', 'VI').data._array, 'schur_eigen n33 V');
  const [D, B] = L.eigen_balance_pre(arr('bal_batch_2x3x7_p2', 'A'), 2);
  assert.deepStrictEqual(Array.from(D.shape), [2, 3, 7]);
  sameValues(D.data, arr('bal_batch_2x3x7_p2', 'D').data, 'eigen_balance_pre D');
  sameValues(B.data, arr('bal_batch_2x3x7_p2', 'B').data, 'eigen_balance_pre B');
  sameValues(L.eigen_balance_pre(arr('bal_graded_7_pinf', 'A'), Infinity)[1].data, arr('bal_graded_7_pinf', 'B').data, 'eigen_balance_pre inf');
  const W = L.eigen_balance_post(arr('post_7', 'D'), arr('post_7', 'V')), Wr = arr('post_7', 'W').data._array;
  assert(W.data instanceof Complex128Array);
  for (let i = 0; i < Wr.length; i++) assert(Math.abs(W.data._array[i] - Wr[i]) <= 4 * Number.EPSILON, 'eigen_balance_post entry ' + i);
  // device-resident round trip
  const Vd = L.schur_eigen(L.to_device(new HostNDArray(Int32Array.of(N, N), eye)), L.to_device(arr('n33', 'T')))[1];
  assert(Vd instanceof L.DeviceNDArray);
  sameValues(L.to_host(Vd).data._array, arr('n33', 'VI').data._array, 'schur_eigen n33 on device arrays');
  assert.throws(() => L.schur_eigenvals(arr('throw_real_block', 'T')), /T must not contain real eigenvalued 2x2 blocks\./);
  console.log('node eigvec gpu checks ok');
} else throw new Error('mode');

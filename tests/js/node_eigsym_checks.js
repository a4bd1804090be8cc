'use strict';
/* Node-side checks of eigen_sym / eigenvals_sym through the JS host and the N-API addon. Driven by tests/test_node_eigsym.py.
 *   node node_eigsym_checks.js cpu                              (no GPU: names, enumerability, argument errors)
 *   node node_eigsym_checks.js install <reference dist/nd.js>   (the names on the patched nd.la, not enumerable, Object.keys unchanged)
 *   node node_eigsym_checks.js gpu <cases.json>                 (GPU: the fixtures of tests/golden/eigsym from host arrays and from
 *                                                                DeviceNDArrays inside the bounds of tests/eigsym_common.py; never
 *                                                                reads the reference)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['eigen_sym', 'eigenvals_sym'];
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

function argumentErrors(L, mk) {
  for (const fn of NAMES) {
    assert.throws(() => L[fn](mk([3], Float64Array.of(1, 2, 3))), err => err.message === `${fn}(S): S.ndim must be at least 2.`, fn);
    assert.throws(() => L[fn](mk([2, 3], new Float64Array(6))), err => err.message === `${fn}(S): S must be quadratic.`, fn);
    assert.throws(() => L[fn](mk([2, 2], new Float32Array(4))), err => err instanceof TypeError, fn + ' float32');
  }
}

// the bounds of tests/eigsym_common.py on one matrix: values within 1e-12 nrm of `ref` (descending), residual, orthogonality
function check(name, N, S, ref, lam, V) {
  let nrm = 0; for (const x of S) nrm += x * x; nrm = Math.sqrt(nrm);
  assert.deepStrictEqual(Array.from(lam.shape), [N], name); assert.deepStrictEqual(Array.from(V.shape), [N, N], name);
  const l = lam.data, v = V.data;
  for (let i = 0; i < N; i++) {
    assert(Math.abs(l[i] - ref[i]) <= 1e-12 * nrm, `${name} lambda[${i}]`);
    assert(i === 0 || l[i] <= l[i - 1], `${name} order`);
  }
  let res = 0, orth = 0;
  for (let i = 0; i < N; i++) for (let j = 0; j < N; j++) {
    let s = 0, o = 0;
    for (let k = 0; k < N; k++) { s += S[N * i + k] * v[N * k + j]; o += v[N * k + i] * v[N * k + j]; }
    res += (s - v[N * i + j] * l[j]) ** 2; orth += (o - (i === j ? 1 : 0)) ** 2;
  }
  assert(Math.sqrt(res) <= 1e-12 * nrm, `${name} residual ${Math.sqrt(res)}`);
  assert(Math.sqrt(orth) <= 1e-12 * Math.sqrt(N), `${name} orthogonality ${Math.sqrt(orth)}`);
}

if (mode === 'cpu') {
  for (const fn of NAMES) {
    assert.strictEqual(typeof la[fn], 'function', fn);
    assert.strictEqual(la[fn].name, fn);
    assert(!Object.keys(la).includes(fn) && !Object.prototype.propertyIsEnumerable.call(la, fn), fn + ' must not be enumerable');
  }
  argumentErrors(la, (shape, data) => new la.NDArray(Int32Array.from(shape), data));
  console.log('node eigsym cpu checks ok');
} else if (mode === 'install') {
  const nd = require(process.argv[3]);
  const before = Object.keys(nd.la).join();
  const L = la.install(nd).la;
  for (const fn of NAMES) {
    assert.strictEqual(typeof L[fn], 'function', fn);
    assert.strictEqual(L[fn].name, fn);
    assert(!Object.keys(L).includes(fn) && !Object.prototype.propertyIsEnumerable.call(L, fn), fn + ' must not be enumerable');
  }
  assert.strictEqual(Object.keys(nd.la).join(), before, 'Object.keys(nd.la) changed');
  argumentErrors(L, (shape, data) => new nd.NDArray(Int32Array.from(shape), data));
  console.log('node eigsym install checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  for (const [name, c] of Object.entries(cases)) {
    const N = c.N, data = Float64Array.from(c.S), S = new la.NDArray(Int32Array.of(N, N), data), keep = Float64Array.from(data);
    const [lam, V] = la.eigen_sym(S);
    assert(lam instanceof la.NDArray && V instanceof la.NDArray, name + ' host in, host out');
    check(name, N, data, c.ref, lam, V);
    assert(sameBits(data, keep), name + ': S was written');
    assert(sameBits(la.eigenvals_sym(S).data, lam.data), name + ': eigenvals_sym has other bits');
    const Sd = la.to_device(S), [ld, Vd] = la.eigen_sym(Sd), l2 = la.eigenvals_sym(Sd);
    assert(ld instanceof la.DeviceNDArray && Vd instanceof la.DeviceNDArray && l2 instanceof la.DeviceNDArray, name + ' device in, device out');
    assert(sameBits(la.to_host(ld).data, lam.data) && sameBits(la.to_host(Vd).data, V.data) && sameBits(la.to_host(l2).data, lam.data), name + ' device bits');
    assert(sameBits(la.to_host(Sd).data, keep), name + ': the device S was written');
    n++;
  }
  const bad = new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 0, NaN, 1));
  assert.throws(() => la.eigen_sym(bad), /NaN or Infinity in its lower triangle/);
  console.log('node eigsym gpu checks ok', n);
} else throw new Error('mode');

'use strict';
/* Node-side checks of eigen_sym_gen / eigenvals_sym_gen through the JS host and the N-API addon. Driven by tests/test_node_sygv.py.
 *   node node_sygv_checks.js cpu                              (no GPU: names, enumerability, argument errors)
 *   node node_sygv_checks.js install <reference dist/nd.js>   (the names on the patched nd.la, not enumerable, Object.keys unchanged)
 *   node node_sygv_checks.js gpu <cases.json>                 (GPU: single-member catalogue cases of tests/sygv_common.py from host
 *                                                              arrays and from DeviceNDArrays inside the values bound, with the
 *                                                              same bits; never reads the reference)
 */
const fs = require('fs'), path = require('path');
const la = require(path.join(__dirname, '..', '..', 'nd4js_amd', 'js'));
const assert = require('assert');
const mode = process.argv[2];
const NAMES = ['eigen_sym_gen', 'eigenvals_sym_gen'];
const sameBits = (a, b) => a.length === b.length && Buffer.compare(Buffer.from(a.buffer, a.byteOffset, a.byteLength), Buffer.from(b.buffer, b.byteOffset, b.byteLength)) === 0;

function argumentErrors(L, mk) {
  const eye = mk([2, 2], Float64Array.of(1, 0, 0, 1));
  for (const fn of NAMES) {
    assert.throws(() => L[fn](mk([3], Float64Array.of(1, 2, 3)), eye), err => err.message === `${fn}(A,B): A.ndim must be at least 2.`, fn);
    assert.throws(() => L[fn](eye, mk([3], Float64Array.of(1, 2, 3))), err => err.message === `${fn}(A,B): B.ndim must be at least 2.`, fn);
    assert.throws(() => L[fn](mk([2, 3], new Float64Array(6)), eye), err => err.message === `${fn}(A,B): A must be quadratic.`, fn);
    assert.throws(() => L[fn](eye, mk([2, 3], new Float64Array(6))), err => err.message === `${fn}(A,B): B must be quadratic.`, fn);
    assert.throws(() => L[fn](mk([2, 2], new Float32Array(4)), eye), err => err instanceof TypeError, fn + ' float32');
    assert.throws(() => L[fn](eye, mk([3, 3], new Float64Array(9))), err => /B\.shape must be A\.shape or A\.shape\.slice\(-2\)/.test(err.message), fn + ' shapes');
    assert.throws(() => L[fn](mk([2, 2, 2], new Float64Array(8)), mk([3, 2, 2], new Float64Array(12))), err => /B\.shape must be/.test(err.message), fn + ' batch shapes');
    assert.throws(() => L[fn](eye, eye, {algo: 'qr'}), err => err.message === `${fn}(A,B, {algo}): algo must be 'dc' or 'jacobi'.`, fn + ' algo');
  }
}

// the values bound of tests/sygv_common.py: |lambda^_i - lambda_i| <= 1e-12 (||A||_F / sigma_min + kappa |lambda_i|), descending
function check(name, c, lam) {
  assert.deepStrictEqual(Array.from(lam.shape), [c.N], name);
  const l = lam.data;
  for (let i = 0; i < c.N; i++) {
    assert(Math.abs(l[i] - c.ref[i]) <= 1e-12 * (c.fro_A / c.sigma_min + c.kappa * Math.abs(c.ref[i])), `${name} lambda[${i}]`);
    assert(i === 0 || l[i] <= l[i - 1], `${name} order`);
  }
}

if (mode === 'cpu') {
  for (const fn of NAMES) {
    assert.strictEqual(typeof la[fn], 'function', fn);
    assert.strictEqual(la[fn].name, fn);
    assert(!Object.keys(la).includes(fn) && !Object.prototype.propertyIsEnumerable.call(la, fn), fn + ' must not be enumerable');
  }
  argumentErrors(la, (shape, data) => new la.NDArray(Int32Array.from(shape), data));
  console.log('node sygv cpu checks ok');
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
  console.log('node sygv install checks ok');
} else if (mode === 'gpu') {
  const cases = JSON.parse(fs.readFileSync(process.argv[3]));
  let n = 0;
  for (const [name, c] of Object.entries(cases)) {
    const N = c.N, da = Float64Array.from(c.A), db = Float64Array.from(c.B), ka = Float64Array.from(da), kb = Float64Array.from(db);
    const A = new la.NDArray(Int32Array.of(N, N), da), B = new la.NDArray(Int32Array.of(N, N), db);
    for (const opts of (N <= 128 ? [undefined, {algo: 'dc'}, {algo: 'jacobi'}] : [undefined])) {
      const [lam, X] = la.eigen_sym_gen(A, B, opts);
      assert(lam instanceof la.NDArray && X instanceof la.NDArray, name + ' host in, host out');
      assert.deepStrictEqual(Array.from(X.shape), [N, N], name);
      check(name, c, lam);
      assert(sameBits(da, ka) && sameBits(db, kb), name + ': an input was written');
      assert(sameBits(la.eigenvals_sym_gen(A, B, opts).data, lam.data), name + ': eigenvals_sym_gen has other bits');
      const Ad = la.to_device(A), Bd = la.to_device(B), [ld, Xd] = la.eigen_sym_gen(Ad, Bd, opts), l2 = la.eigenvals_sym_gen(Ad, Bd, opts);
      assert(ld instanceof la.DeviceNDArray && Xd instanceof la.DeviceNDArray && l2 instanceof la.DeviceNDArray, name + ' device in, device out');
      assert(sameBits(la.to_host(ld).data, lam.data) && sameBits(la.to_host(Xd).data, X.data) && sameBits(la.to_host(l2).data, lam.data), name + ' device bits');
      assert(sameBits(la.to_host(Ad).data, ka) && sameBits(la.to_host(Bd).data, kb), name + ': a device input was written');
      assert.throws(() => la.eigen_sym_gen(Ad, B, opts), TypeError, name + ': mixed sides');
    }
    n++;
  }
  // one B for a stack of A: the same bits as the stacked call
  const c = cases.gram_3, N = 3;
  const A2 = new la.NDArray(Int32Array.of(2, N, N), Float64Array.from(c.A.concat(c.A))), B1 = new la.NDArray(Int32Array.of(N, N), Float64Array.from(c.B));
  const B2 = new la.NDArray(Int32Array.of(2, N, N), Float64Array.from(c.B.concat(c.B)));
  const [ls, Xs] = la.eigen_sym_gen(A2, B1), [lt, Xt] = la.eigen_sym_gen(A2, B2);
  assert.deepStrictEqual(Array.from(ls.shape), [2, N]);
  assert(sameBits(ls.data, lt.data) && sameBits(Xs.data, Xt.data), 'one B for every member');
  const eye = new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 0, 0, 1));
  assert.throws(() => la.eigen_sym_gen(eye, new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 0, 0, 0))), /B is not positive definite\. \(matrix 0\)/);
  assert.throws(() => la.eigen_sym_gen(new la.NDArray(Int32Array.of(2, 2), Float64Array.of(1, 0, NaN, 1)), eye), /L\^-1 A L\^-T is not finite/);
  console.log('node sygv gpu checks ok', n);
} else throw new Error('mode');
